"""CPU-side checks of the device metadetection mosaic (seam 19): the host functions of pyimcom_amd.metamosaic and the numpy restatement
(tests/metamosaic_reference.py) against tests/golden/metamosaic.npz, which holds what the reference's own statements gave; csrc/mosaic_core.h
as a host program under the sanitizers; the null-context refusal of the new entries.  Everything is compared with ``==``."""

import json
import os
import subprocess
import types

import numpy as np
import pytest

from tests import metamosaic_reference as MR
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "metamosaic.npz"))
META = json.loads(str(G["meta"]))
CFG = META["cfg"]
MOSAICS = {m["name"]: m for m in META["mosaics"]}
CAPS = [c["name"] for c in META["caps"]]
ENTRIES = ["imcom_mosaic_paste", "imcom_mosaic_mask_cut", "imcom_mosaic_caps"]


def cfg_like():
    return types.SimpleNamespace(**CFG)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def blocks_of(case):
    """blocks[(in_x, in_y)] of a mosaic case as the generator filled its files: dict(primary, fidelity, sigma, fid_bels, sig_bels)."""
    out = {}
    for key, (fb, sb) in META["bels"].items():
        bx, by = (int(v) for v in key.split(","))
        p = G[f"block_{bx}_{by}_primary"][: case["nlayer"]]
        fid = G[f"block_{bx}_{by}_fidelity"]
        out[(bx, by)] = {"primary": MR.to_float64(p) if case["dtype"] == "float64" else p, "fidelity": MR.to_uint8(fid) if case["variant"] == "u8" else fid,
                         "sigma": G[f"block_{bx}_{by}_sigma"], "fid_bels": fb, "sig_bels": sb}
    return out


def test_the_fixture_holds_the_cases_the_issue_lists():
    m = MOSAICS
    assert len(m["interior"]["windows"]) == 9 and m["interior"]["nlayer"] == 3
    assert (m["corner"]["ix"], m["corner"]["iy"]) == (0, CFG["nblock"] - 1) and len(m["corner"]["windows"]) == 4
    assert len(m["bbox"]["windows"]) == 6 and int(G["bbox_mask"][:, 64:].all()) == 1 and not G["bbox_image"][:, :, 64:].any()
    assert m["ext10"]["trunc"] == 22 and m["ext10"]["Nside"] == 52 and m["ext0"]["Nside"] == 32 and len(m["ext0"]["windows"]) == 1
    wx = {(w[6], w[7]) for w in m["ext10"]["windows"]}
    assert (30, 40) in wx and (8, 18) in wx  # cx + sxmin < 0 and cx + sxmax > Nside were both taken
    assert {c["nlayer"] for c in m.values()} == {1, 3} and {c["dtype"] for c in m.values()} == {"float32", "float64"}
    assert G["block_1_2_fidelity"].dtype == np.uint16 and (G["block_1_2_fidelity"] == 0).any()
    assert G["block_1_2_sigma"].dtype == np.int16 and (G["block_1_2_sigma"] < 0).any()
    assert np.isnan(META["bels"]["1,1"][0]) and np.isnan(META["bels"]["0,2"][1]) and META["bels"]["2,2"][0] == -0.0002 and META["units"]["2,2"][0] == "0.2mB"
    assert np.isnan(G["interior_fidelity"]).any() and np.isnan(G["interior_noise"]).any()
    assert np.isnan(G["interior_image"]).any() and np.isinf(G["interior_image"]).any()
    assert set(CAPS) >= {"inside", "left", "right", "bottom", "top", "corner", "outside", "r0", "between", "on_centre", "overlap", "huge", "none", "random"}
    by_name = {c["name"]: c for c in META["caps"]}
    assert by_name["between"]["hits"] == 0 and by_name["on_centre"]["hits"] == 1 and by_name["huge"]["hits"] == 96 * 96 and by_name["random"]["n"] == 1000
    assert all(c["margin"] is None or c["margin"] > META["margin"] for c in META["caps"]) and all(s["edge"] >= META["edge"] for s in META["sky"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "metamosaic.npz")) < 700_000


def test_cap_cases_keep_their_margin():
    """|d^2 - r^2| > 1e-12 r^2 for every tested pixel (np.longdouble): every faithful hypot decides alike."""
    for name in CAPS:
        x, y, r = G[f"caps_{name}_xyr"]
        assert MR.cap_margin(x, y, r, 96) > META["margin"], name


@pytest.mark.parametrize("name", sorted(MOSAICS))
def test_block_windows_and_header_match_the_reference(name):
    from pyimcom_amd import metamosaic as M

    c = MOSAICS[name]
    for cfg in (cfg_like(), dict(CFG)):
        trunc, Nside, wins = M.block_windows(cfg, c["ix"], c["iy"], c["bbox"], c["extpix"])
        assert (trunc, Nside) == (c["trunc"], c["Nside"]) and [list(w) for w in wins] == c["windows"]
        assert M.mosaic_header(cfg, c["ix"], c["iy"], trunc) == c["header"]
    assert MR.windows(CFG, c["ix"], c["iy"], c["bbox"], c["extpix"]) == (c["trunc"], c["Nside"], [tuple(w) for w in c["windows"]])


@pytest.mark.parametrize("name", sorted(MOSAICS))
def test_restatement_builds_the_reference_arrays(name):
    c = MOSAICS[name]
    image, fid, noise, mask = MR.build(CFG, c["ix"], c["iy"], c["nlayer"], np.dtype(c["dtype"]), blocks_of(c), c["bbox"], c["extpix"])
    assert image.dtype == G[name + "_image"].dtype and np.array_equal(bits(image), bits(G[name + "_image"]))
    assert np.array_equal(bits(fid), bits(G[name + "_fidelity"])) and np.array_equal(bits(noise), bits(G[name + "_noise"]))
    assert np.array_equal(mask, G[name + "_mask"])


def test_units_parse_as_the_reference_parses_them():
    for key, (fb, sb) in META["bels"].items():
        fu, fc, su, sc = META["units"].get(key, [MR.FID_UNIT, "x", MR.SIG_UNIT, "x"])
        for got, want in ((MR.unit_to_bels(fu, fc), fb), (MR.unit_to_bels(su, sc), sb)):
            assert got == want or (np.isnan(got) and np.isnan(want))


def test_restatement_of_the_mask_methods():
    mask = G["interior_mask"].copy()
    mask = np.logical_or(G["interior_fidelity"] < META["cuts"]["fidelitymin"], mask)
    assert np.array_equal(mask, G["cut_fidelity"]) and mask.sum() > G["interior_mask"].sum()
    mask = np.logical_or(G["interior_noise"] > META["cuts"]["noisemax"], mask)
    assert np.array_equal(mask, G["cut_noise"]) and mask.sum() > G["cut_fidelity"].sum()
    assert np.array_equal(np.logical_or(G["extramask"], mask), G["cut_extra"])


@pytest.mark.parametrize("name", CAPS)
def test_restatement_of_the_circles(name):
    x, y, r = G[f"caps_{name}_xyr"]
    assert np.array_equal(MR.caps(np.zeros((96, 96), dtype=bool), x, y, r), G[f"caps_{name}_mask"])


@pytest.mark.parametrize("k", range(len(META["shear"])))
def test_shear_geometry_matches_the_reference(k):
    from pyimcom_amd import metamosaic as M

    s, c = META["shear"][k], MOSAICS["interior"]
    g = M.shear_geometry(cfg_like(), c["ix"], c["iy"], c["trunc"], s["N"], None if s["jac"] is None else np.array(s["jac"]), s["psfgrow"], s["oversamp"], META["stem"])
    assert np.array_equal(g["opos"], G[f"shear_{s['name']}_opos"]) and np.array_equal(g["J"], G[f"shear_{s['name']}_J"])
    assert g["sigma"] * np.sqrt(8 * np.log(2)) == s["samp"] and MR.plain(g["C"]) == s["C"]
    assert MR.plain(g["header"]) == s["header"] and MR.plain(g["pardict"]) == s["pars"] and list(g["pardict"]) == list(s["pars"])
    assert MR.plain((g["xref"] - 1, g["yref"] - 1)) == s["ref"] and np.sqrt(8.0 * np.log(2)) * g["pardict"]["SIGMAOUT"][0] == s["psf_fwhm"]


@pytest.mark.parametrize("k", range(len(META["orig"])))
def test_orig_geometry_matches_the_reference(k):
    from pyimcom_amd import metamosaic as M

    o = META["orig"][k]
    c = MOSAICS[o["mosaic"]]
    g = M.orig_geometry(cfg_like(), c["ix"], c["iy"], c["trunc"], o["N"], META["stem"])
    overfills = g["opos"] < 0 or g["opos"] + g["N"] > 3 * CFG["n1"] * CFG["n2"] - 2 * c["trunc"]
    assert overfills == o["raises"]
    if o["raises"]:
        return
    assert G[f"orig{k}_mask"].shape == (g["N"], g["N"])
    assert MR.plain(g["header"]) == o["header"] and MR.plain(g["pardict"]) == o["pars"] and list(g["pardict"]) == list(o["pars"])
    assert MR.plain((g["xref"] - 1, g["yref"] - 1)) == o["ref"] and np.sqrt(8.0 * np.log(2)) * g["pardict"]["SIGMAOUT"][0] == o["psf_fwhm"]
    src = G[o["mosaic"] + "_image"][:, g["opos"]:g["opos"] + g["N"], g["opos"]:g["opos"] + g["N"]]
    assert np.array_equal(bits(src if o["select_layers"] is None else src[o["select_layers"]]), bits(G[f"orig{k}_image"]))


def test_a_psf_that_is_not_gaussian_is_refused():
    from pyimcom_amd import metamosaic as M

    with pytest.raises(ValueError, match="only works on GAUSSIAN"):
        M._require_gaussian(dict(CFG, outpsf="AIRYOBSC"))


# ---- the core as a host program ---------------------------------------------------------------------------------------------------------

def _f64_bits(v):
    return np.array([v], dtype=np.float64).view(np.int64)[0]


def _jobs_file(path):
    jobs, nwin, ncaps, ndb = [], 0, 0, 0
    for c in META["mosaics"]:
        for w in c["windows"]:
            jobs.append([0] + [w[4], w[5], w[6], w[7], w[9], w[8], META["block_side"], META["block_side"], c["Nside"]])
            nwin += 1
    jobs.append([0, 3, 2054, 5, 2053, 11, 8, 2060, 2061, 2112])  # the large window of the GPU test (2051 x 2048 at an odd offset)
    jobs.append([0, 0, 0, 0, 0, 0, 0, 48, 48, 96])                 # an empty window
    nwin += 2
    for name in CAPS:
        xyr, mask = G[f"caps_{name}_xyr"], G[f"caps_{name}_mask"]
        packed = np.zeros((mask.size + 7) // 8 * 8, dtype=np.uint8)
        packed[: mask.size] = mask.ravel()
        jobs.append(np.concatenate(([1, 96, xyr.shape[1]], np.ascontiguousarray(xyr.T).view(np.int64).ravel(), packed.view(np.int64))))
        ncaps += 1
    clamp = np.array([[1e300, -1e300, 50.0, 50.0], [40.0, 40.0, 1e300, -1e300], [5.0, 5.0, 5.0, 1e308]])  # positions and radii far beyond any integer
    want = MR.caps(np.zeros((96, 96), dtype=bool), *clamp)  # (three empty boxes, and one circle that holds the mosaic)
    assert want.all()
    jobs.append(np.concatenate(([1, 96, 4], np.ascontiguousarray(clamp.T).view(np.int64).ravel(), want.astype(np.uint8).ravel().view(np.int64))))
    ncaps += 1
    for key, (fb, sb) in META["bels"].items():
        bx, by = key.split(",")
        for kind, codes, bels, div, dbs in ((1, G[f"block_{bx}_{by}_fidelity"], fb, 0, MR.decibels(G[f"block_{bx}_{by}_fidelity"], fb, -0.1)),
                                            (2, G[f"block_{bx}_{by}_sigma"], sb, 1, MR.decibels(G[f"block_{bx}_{by}_sigma"], sb, 0.1)),
                                            (0, MR.to_uint8(G[f"block_{bx}_{by}_fidelity"]), fb, 0, MR.decibels(MR.to_uint8(G[f"block_{bx}_{by}_fidelity"]), fb, -0.1))):
            u, first = np.unique(codes.ravel(), return_index=True)
            pairs = np.stack((u.astype(np.int64), dbs.ravel()[first].view(np.uint32).astype(np.int64)), axis=1)
            jobs.append(np.concatenate(([2, kind, div, _f64_bits(bels), len(u)], pairs.ravel())))
            ndb += len(u)
    np.concatenate([np.array([len(jobs)], dtype=np.int64)] + [np.asarray(j, dtype=np.int64) for j in jobs]).tofile(path)
    return nwin, ncaps, ndb


def test_decibels_of_the_restatement_are_the_golden_values():
    """(what the native check is given as the expected float32 values)"""
    c = MOSAICS["interior"]
    for w in c["windows"]:
        fb, sb = META["bels"][f"{w[2]},{w[3]}"]
        src, dst = (slice(w[4], w[5]), slice(w[6], w[7])), (slice(w[4] + w[9], w[5] + w[9]), slice(w[6] + w[8], w[7] + w[8]))
        assert np.array_equal(bits(MR.decibels(G[f"block_{w[2]}_{w[3]}_fidelity"][src], fb, -0.1)), bits(G["interior_fidelity"][dst]))
        assert np.array_equal(bits(MR.decibels(G[f"block_{w[2]}_{w[3]}_sigma"][src], sb, 0.1)), bits(G["interior_noise"][dst]))


def test_native_core_against_the_fixture_under_sanitizers(tmp_path):
    exe, jobs = tmp_path / "mosaic_check", tmp_path / "jobs.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "mosaic_check.cpp"), "-o", str(exe)])
    nwin, ncaps, ndb = _jobs_file(str(jobs))
    out = subprocess.run([str(exe), str(jobs)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["windows", "splits", "caps", "pixels", "decibels"]
    assert int(rows[0][1]) == nwin and int(rows[2][1]) == ncaps and int(rows[4][1]) == ndb and all(int(r[2]) == 0 and int(r[1]) > 0 for r in rows), rows


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_null_context_is_refused_before_anything_else(name):
    import ctypes as C

    from pyimcom_amd import _lib

    def null(t):
        if t in (C.c_double, C.c_float):
            return 0.0
        return 0 if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" else None

    assert getattr(_lib.lib, name)(*[null(t) for t in _lib.SIGNATURES[name]]) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()
