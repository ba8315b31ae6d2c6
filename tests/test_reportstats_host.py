"""The validation report's statistics without a device: the numpy restatement (tests/reportstats_reference.py) against the reference's own
outputs recorded in tests/golden/reportstats.npz, the host's percentile and code-table steps of pyimcom_amd.reportstats against numpy, and
the host-compilable core of the kernels (csrc/quantiles_core.h) against the standard library, built with the address and
undefined-behaviour sanitizers as a stand-alone program (tests/native/quantiles_check.cpp)."""

import os
import subprocess

import numpy as np
import pytest

from tests import reportstats_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "reportstats.npz"))


def golden_frames():
    return {(int(bx), int(by)): G[f"frames_{bx}_{by}"] for bx, by in G["blocks"]}


def test_restated_inputs_are_the_recorded_ones():
    frames, want = R.mosaic(), golden_frames()
    assert sorted(frames) == sorted(want) and R.MISSING not in want and len(want) == R.NBLOCK ** 2 - 1
    assert all(np.array_equal(frames[k].view(np.uint32), want[k].view(np.uint32)) for k in want)
    starmap, x, y, sigma, neff = R.star_frame()
    assert np.array_equal(starmap, G["starmap"]) and np.array_equal(x, G["x"]) and np.array_equal(y, G["y"])
    assert np.array_equal(sigma, G["sigma"]) and sigma.dtype == np.int16 and np.array_equal(neff, G["neff"]) and neff.dtype == np.uint16


def test_layer_percentiles_of_the_restatement_are_the_references():
    got = R.layer_percentiles(golden_frames())
    assert got.dtype == np.float32 and np.array_equal(got, G["pcarray"])
    assert np.signbit(G["pcarray"][1, 6])  # the reference's sort leaves a -0.0 at the median of the tied layer: equal to 0.0, not the same bits


def test_rings_of_the_restatement_are_the_references():
    vals = R.ring_values(G["starmap"], G["x"], G["y"], int(G["rpix"]))
    assert np.array_equal([v.size for v in vals], G["ring_counts"])
    assert np.array_equal(np.concatenate(vals), G["ring_vals"])
    # the cases the frame is there for: a star off the frame adds nothing, clipped boxes lose pixels, overlapping boxes count a pixel twice
    alone = R.ring_values(G["starmap"], G["x"][6:7], G["y"][6:7], int(G["rpix"]))
    assert sum(v.size for v in alone) == 0
    full = sum(v.size for v in R.ring_values(G["starmap"], G["x"][:1], G["y"][:1], int(G["rpix"])))
    for k in (2, 3, 4, 5):
        assert 0 < sum(v.size for v in R.ring_values(G["starmap"], G["x"][k:k + 1], G["y"][k:k + 1], int(G["rpix"]))) < full
    assert np.hypot(G["x"][7] - G["x"][8], G["y"][7] - G["y"][8]) < int(G["rpix"])


def test_histograms_of_the_restatement_are_the_references():
    assert float(G["sigma_bels"]) == R.unit_to_bels(*R.SIGMA_UNIT) and float(G["neff_bels"]) == R.unit_to_bels(*R.NEFF_UNIT)
    c, size, gt = R.histogram(G["sigma"], float(G["sigma_bels"]), True, 0.02, 100, int(G["bd"]))
    assert np.array_equal(c, G["countnoise"][:, 1]) and (size, gt) == tuple(G["totals"][:2])
    c, size, gt = R.histogram(G["neff"], float(G["neff_bels"]), False, 0.1, 100, int(G["bd"]), int(G["nscale"]))
    assert np.array_equal(c, G["countneff"][:, 1]) and (size, gt) == tuple(G["totals"][2:])
    assert G["totals"][1] >= 1 and G["totals"][3] >= 1  # something is off scale high in both


@pytest.fixture(scope="module")
def RS():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import reportstats

    return reportstats


def test_percentile_step_is_numpys_for_every_size(RS):
    rng = np.random.default_rng(5)
    for n in range(1, 201):
        a = rng.standard_normal(n).astype(np.float32)
        if n % 4 == 0:
            a = np.round(a * 2) / np.float32(4)  # ties
        s = np.sort(a)
        for q in RS.RING_PCTILES:
            lo, hi, gamma = RS.percentile_ranks(n, q, np.float32)
            got, want = RS.percentile_from_order_statistics(s[lo], s[hi], gamma), np.percentile(a, q)
            assert type(got) is type(want) and got == want, (n, q, got, want)
    a = np.array([1.0, np.nan, 3.0], dtype=np.float32)
    assert np.isnan(RS.percentile_from_order_statistics(a[0], a[2], np.float32(0.5), any_nan=True)) and np.isnan(np.percentile(a, 50))


def test_ring_percentiles_from_two_order_statistics_are_the_references(RS):
    vals, at = G["ring_vals"], np.concatenate([[0], np.cumsum(G["ring_counts"])])
    for j in range(int(G["rpix"])):
        s = np.sort(vals[at[j]:at[j + 1]])
        for k, q in enumerate(RS.RING_PCTILES):
            lo, hi, gamma = RS.percentile_ranks(s.size, q, np.float32)
            assert RS.percentile_from_order_statistics(s[lo], s[hi], gamma) == G["ring_percentiles"][j, k]


def test_layer_step_is_the_references(RS):
    for nsize in (2, 3, 9216, 8_493_465_600):
        for p in RS.LAYER_PCTILES:
            p1, frac = RS._layer_position(nsize, p)
            assert 0 <= p1 <= nsize - 2 and 0.0 <= frac <= 1.0
    assert RS._layer_position(9216, 100) == (9214, 1.0) and RS._layer_position(9216, 0) == (0, 0.0)
    with pytest.raises(ValueError, match="fewer than 2"):
        RS.layer_percentiles({(0, 0): np.zeros((1, 1, 1), dtype=np.float32)}, 1, 0, 1)


def test_code_table_bins_every_code_as_the_reference_bins_a_pixel(RS):
    for dtype, bels, half, width in ((np.int16, float(G["sigma_bels"]), True, 0.02), (np.uint16, float(G["neff_bels"]), False, 0.1)):
        codes = RS._all_codes(dtype)
        assert codes.dtype == dtype and np.array_equal(codes.view(np.uint16), np.arange(65536))
        with np.errstate(all="ignore"):
            v = 10 ** (0.5 * bels * codes) if half else 10 ** (bels * codes * 1)
        t = RS.code_bin_table(v, width, 100)
        for j in (0, 1, 50, 99):
            assert np.array_equal((t & 127 == j) & (t != 255), np.logical_and(v / width >= j, v / width < j + 1))
        assert np.array_equal((t == 100) | ((t >= 128) & (t != 255)), v >= width * 100)
        # through the table, the golden maps give the golden counts (what the device does, in numpy)
        m = G["sigma" if half else "neff"]
        bd = int(G["bd"])
        tv = t[m[bd:-bd, bd:-bd].view(np.uint16)]
        assert np.array_equal(np.bincount(tv[tv < 100], minlength=100), G["countnoise" if half else "countneff"][:, 1])
    nan_table = RS.code_bin_table(np.full(65536, np.nan), 0.02, 100)
    assert (nan_table == 255).all()
    v = np.array([1.98, 1.9799999, 2.0, 5.0, -1.0] + [0.0] * 65531)  # 99 bins: a value may be in the last bin and off scale high at once
    t = RS.code_bin_table(v, 0.02, 99)
    for i in range(5):
        bins = [j for j in range(99) if v[i] / 0.02 >= j and v[i] / 0.02 < j + 1]
        high = v[i] >= 0.02 * 99
        assert t[i] == (bins[0] + 128 * high if bins else 99 if high else 255), (i, t[i], bins, high)
    assert t[5] == 0


def test_native_core_against_the_standard_library_under_sanitizers(tmp_path):
    exe = tmp_path / "quantiles_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "quantiles_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[:2] for r in rows] == [["select", "float32"], ["select", "float64"], ["groups", "most"], ["rings", "float64"]]
    assert all(int(r[2]) > 0 and int(r[3]) == 0 for r in rows), rows
    assert int(rows[2][2]) >= 13  # more live groups than a launch's tile of 8: the grouping is exercised
