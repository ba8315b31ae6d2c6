"""The star catalog without a device: the numpy restatement (tests/starcat_reference.py) against what the reference's own statements gave
with it (tests/golden/starcat.npz), the restated adaptive moments against analysis (a sampled elliptical Gaussian is its own fixed point)
and, where GalSim is installed, against ``FindAdaptiveMom`` itself; the host-compilable core of the kernels (csrc/starmom_core.h) built with
the address and undefined-behaviour sanitizers as a stand-alone program (tests/native/starmom_check.cpp); and the host side of
pyimcom_amd.starcat (the code table of the fidelity map, the selection of stars)."""

import os
import subprocess

import numpy as np
import pytest

from tests import starcat_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "starcat.npz"))
BDS = [int(b) for b in G["bds"]]


def test_restated_inputs_are_the_recorded_ones():
    F = R.fixture_frame()
    x, y = R.star_positions()
    assert np.array_equal(x, G["x"]) and np.array_equal(y, G["y"]) and float(G["forced_scale"]) == R.FORCED_SCALE and float(G["bels"]) == R.BELS
    for key in ("frame", "fid", "inweight", "uc", "sigma", "tsum", "neff"):
        assert F[key].dtype == G[key].dtype and np.array_equal(F[key], G[key]), key
    assert G["frame"].dtype == np.float32 and G["frame"].shape == (96, 96) and G["fid"].dtype == np.uint16
    assert (np.rint(x[8]), np.rint(y[8])) == (2, 93)  # the cut that hangs over two edges


@pytest.mark.parametrize("bd", BDS)
def test_restatement_is_the_golden(bd):
    """The whole catalog row in numpy equals, bit for bit, what the reference's statements computed with the restated moments."""
    F = {k: G[k] for k in ("frame", "fid", "inweight", "uc", "sigma", "tsum", "neff")}
    fits = G[f"fits_{bd}"]
    x, y = G["x"][fits], G["y"][fits]
    cat = R.catalog(F["frame"], x, y, bd, int(G["bd2"]), float(G["forced_scale"]), (F["fid"], float(G["bels"])), F["inweight"], int(G["n2"]), F["uc"], F["sigma"],
                    F["tsum"], F["neff"], ra=G["ra"][fits], dec=G["dec"][fits])
    assert list(G["columns"]) == R.COLUMNS and cat.shape == G[f"cat_{bd}"].shape
    assert np.array_equal(cat, G[f"cat_{bd}"])
    emp = R.catalog(F["frame"], x, y, bd, int(G["bd2"]), float(G["forced_scale"]), (F["fid"], float(G["bels"])), F["inweight"], int(G["n2"]), F["uc"], None, F["tsum"],
                    None, empirical=True, ra=G["ra"][fits], dec=G["dec"][fits])
    assert np.array_equal(emp, G[f"cat_empirical_{bd}"])
    ok = G[f"mom_{bd}"][fits, 10] == 0
    assert np.all(emp[ok, R.COLUMNS.index("MEAN_SIGMA")] == -1) and np.all(emp[ok, R.COLUMNS.index("STD_TSUM")] == 0) and np.all(emp[~ok, 4:] == 0)
    # the rows of gen_starcube_nonoise: the same columns 10-19 where both ran, and the padded cuts
    rows = G[f"rows_{bd}"]
    assert np.array_equal(rows[fits, 10:20], G[f"cat_{bd}"][:, 4:14]) and np.array_equal(rows[fits, 20:22], G[f"cat_{bd}"][:, 14:16])
    xi, yi = np.rint(G["x"]).astype(int), np.rint(G["y"]).astype(int)
    for k in range(len(xi)):
        cut = R.cut(F["frame"], xi[k], yi[k], bd)
        assert np.array_equal(cut, G[f"cube_{bd}"][k])
        m = R.find_adaptive_mom(cut)
        assert (m.moments_status, m.moments_n_iter) == (int(G[f"mom_{bd}"][k, 10]), int(G[f"mom_{bd}"][k, 9]))
        if m.moments_status == 0:
            assert m.moments_amp == rows[k, 10] and m.moments_sigma == rows[k, 13] and m.moments_rho4 == G[f"mom_{bd}"][k, 8]
        else:
            assert np.all(rows[k, 10:] == 0)


def test_statuses_of_the_failing_stars():
    mom = {bd: G[f"mom_{bd}"] for bd in BDS}
    assert mom[40][6, 10] == R.STATUS_TOO_LARGE  # drawn 20 px from its nominal position: the shift passes max_ashift
    assert mom[40][5, 10] == R.STATUS_OK and abs(mom[40][5, 1] - 28.0) < 1e-3  # drawn 12 px off: converges on the star, 12 px from the centre
    for bd in (4, 8):
        cut = R.cut(G["frame"], 42, 42, bd)
        assert not cut.any() and mom[bd][7, 10] == R.STATUS_NAN and mom[bd][7, 9] == 1  # empty sky: A = 0 in the first iteration
    assert mom[40][4, 10] == R.STATUS_OK and mom[40][4, 0] < 0  # a negative star converges with a negative amplitude
    assert all(mom[bd][8, 10] == R.STATUS_OK for bd in BDS)  # over two frame edges
    assert R.find_adaptive_mom(np.ones((79, 79))).moments_status == R.STATUS_OK  # a flat image converges (on the weight the bounds allow)
    p = R.Params(max_mom2_iter=3)
    assert R.find_adaptive_mom(R.cut(G["frame"], 42, 14, 40), p).moments_status == R.STATUS_TOO_MANY


@pytest.mark.parametrize("flux,sig,e1,e2,cx,cy", [(3.0, 2.5, 0.0, 0.0, 39.0, 39.0), (1.7, 3.1, 0.25, -0.1, 39.3, 38.6), (-2.0, 2.0, -0.3, 0.2, 38.51, 39.49)])
def test_sampled_gaussian_is_its_own_fixed_point(flux, sig, e1, e2, cx, cy):
    m = R.find_adaptive_mom(R.draw_star(79, cx, cy, flux, sig, e1, e2, 0.0))
    assert m.error_message == "" and m.moments_n_iter < 40
    assert abs(m.moments_amp - flux) < 1e-8 * abs(flux) and abs(m.moments_sigma - sig) < 1e-8 * sig
    assert abs(m.moments_centroid.x - (cx + 1)) < 1e-8 * sig and abs(m.moments_centroid.y - (cy + 1)) < 1e-8 * sig
    assert abs(m.observed_shape.e1 - e1) < 1e-8 and abs(m.observed_shape.e2 - e2) < 1e-8
    assert abs(m.moments_rho4 - 2.0) < 1e-6  # <rho^4> of a Gaussian under its own weight


def test_restatement_against_galsim_where_it_is_installed():
    galsim = pytest.importorskip("galsim")
    xi, yi = np.rint(G["x"]).astype(int), np.rint(G["y"]).astype(int)
    for bd in BDS:
        for k in range(len(xi)):
            cut = np.ascontiguousarray(G[f"cube_{bd}"][k])
            want, got = galsim.Image(cut).FindAdaptiveMom(strict=False), R.find_adaptive_mom(cut)
            assert (want.error_message == "") == (got.error_message == ""), (bd, k, want.error_message, got.error_message)
            if got.error_message == "":
                sc = G[f"scale_{bd}"][k]
                assert want.moments_n_iter == got.moments_n_iter
                assert abs(want.moments_amp - got.moments_amp) <= 1e-6 * sc[0] and abs(want.moments_sigma - got.moments_sigma) <= 1e-6 * sc[3]  # (float32 images in GalSim)
                assert abs(want.moments_centroid.x - got.moments_centroid.x) <= 1e-6 * sc[1] and abs(want.moments_centroid.y - got.moments_centroid.y) <= 1e-6 * sc[2]
                assert abs(want.observed_shape.g1 - got.observed_shape.g1) <= 1e-6 and abs(want.observed_shape.g2 - got.observed_shape.g2) <= 1e-6
                assert abs(want.moments_rho4 - got.moments_rho4) <= 1e-5


def _write_dump(path):
    TRACES = sorted(tuple(int(v) for v in key.split("_")[1:3]) for key in G.files if key.startswith("trace_") and key.endswith("_pre"))
    lines = [f"N {len(TRACES)}"]
    xi, yi = np.rint(G["x"]).astype(int), np.rint(G["y"]).astype(int)
    for k, bd in TRACES:
        pre, post, rows, sums = (G[f"trace_{k}_{bd}_{n}"] for n in ("pre", "post", "rows", "sums"))
        cut = R.cut(G["frame"], xi[k], yi[k], bd)
        lines.append(f"T {cut.shape[0]} {cut.shape[1]} {len(pre)}")
        lines.append(" ".join(repr(float(v)) for v in cut.ravel()))
        for it in range(len(pre)):
            lines.append("P " + " ".join(repr(float(v)) for v in pre[it, :6]) + f" {int(pre[it, 6])} {int(pre[it, 7])}")
            lines += [f"R {r[1]} {r[2]} {r[3]}" for r in rows[rows[:, 0] == it]]
            lines.append("S " + " ".join(repr(float(v)) for v in sums[it]))
            lines.append("Q " + " ".join(repr(float(v)) for v in post[it, :6]) + f" {int(post[it, 6])}")
    path.write_text("\n".join(lines) + "\n")
    return sum(len(G[f"trace_{k}_{bd}_pre"]) for k, bd in TRACES)


def test_native_core_under_sanitizers(tmp_path):
    exe, dump = tmp_path / "starmom_check", tmp_path / "starmom_dump.txt"
    niter = _write_dump(dump)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "starmom_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[:2] for r in rows] == [["ranges", "recorded"], ["ranges", "brute"], ["sums", "recorded"], ["step", "recorded"], ["endings", "synthetic"]]
    assert all(int(r[2]) > 0 and int(r[3]) == 0 for r in rows), rows
    assert int(rows[0][2]) > 2 * niter and int(rows[3][2]) == 7 * niter and niter > 60


@pytest.fixture(scope="module")
def SC():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import starcat

    return starcat


def test_fidelity_table_is_the_references_expression_on_every_code(SC):
    assert SC.COLUMNS == list(G["columns"]) and SC.STATUS_MESSAGES == R.MESSAGES
    p, q = SC.AdaptiveMomParams(), R.Params()
    assert vars(p) == vars(q)
    for dtype in (np.uint16, np.int16):
        t = SC.fidelity_table(dtype, float(G["bels"]))
        codes = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(dtype)
        assert t.dtype == np.int16 and np.array_equal(t, R.fidelity_map(codes, float(G["bels"])))
    fmap = R.fidelity_map(G["fid"], float(G["bels"]))
    assert np.array_equal(SC.fidelity_table(np.uint16, float(G["bels"]))[G["fid"]], fmap)
    bdpad = int(G["bdpad"])
    want = np.array([np.count_nonzero(fmap[bdpad:-bdpad, bdpad:-bdpad] == fy) for fy in range(81)])
    assert np.array_equal(want, G["fhist"]) and want.sum() > 0 and want[0] > 0
    c = SC.cumulative(G["fhist"])
    assert c.shape == (81, 2) and abs(c[-1, 1] - 1.0) < 1e-15 and np.allclose(c[:, 0].sum(), 1.0)


def test_selection_of_stars_is_the_references(SC):
    x, y, n, bdpad = np.array([9.5, 10.5, 85.4, 85.6, 50.0, 50.0]), np.array([50.0, 50.0, 50.0, 50.0, 9.4, 86.0]), 96, 10
    xi, yi = np.rint(x).astype(np.int16), np.rint(y).astype(np.int16)
    grp = np.where(np.logical_and(np.logical_and(xi >= bdpad, xi < n - bdpad), np.logical_and(yi >= bdpad, yi < n - bdpad)))
    assert np.array_equal(SC.select_stars(x, y, n, bdpad), grp[0]) and list(grp[0]) == [0, 1, 2]
