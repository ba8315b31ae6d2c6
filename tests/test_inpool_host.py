"""CPU-side checks of seam 17 (the input-stamp pool): the numpy restatement (tests/inpool_reference.py) against the golden file that the
reference's own statements wrote (tests/golden/make_golden_inpool.py), the host parts of pyimcom_amd.inpool against the same file, and the
visit-index decode of csrc/partition_core.h against plain loops, as a stand-alone program under the host sanitizers."""

import json
import os
import subprocess

import numpy as np
import pytest

from tests import inpool_reference as P
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "inpool.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def positions(z, name, nside):
    """The golden's positions of image `name` as frames [nside, nside]: NaN where the file holds none (out of range, or never visited)."""
    x, y = np.full(nside * nside, np.nan), np.full(nside * nside, np.nan)
    x[z[f"{name}_inr_idx"]], y[z[f"{name}_inr_idx"]] = z[f"{name}_inr_x"], z[f"{name}_inr_y"]
    return x.reshape(nside, nside), y.reshape(nside, nside)


def variants(meta):
    for name, info in meta["images"].items():
        if info["is_relevant"]:
            yield name, name, info, True if info["masked"] else None
            if info["masked"]:
                yield name, name + "_nomask", info, None


def test_fixture_is_small_and_far_from_every_decision_boundary(gold):
    z, meta = gold
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert meta["nside"] == 190 and meta["n2"] == 8 and meta["n1P"] == 6
    for name, info in meta["images"].items():
        assert info["boundary_distance"] > 1e-6, name
    rel = {k: v["is_relevant"] for k, v in meta["images"].items()}
    assert rel == {"a": True, "b": True, "c": False, "d": False, "a2": True, "s": True}
    assert meta["images"]["s"]["visits"] < 2048 < 3 * 2048 < meta["images"]["a"]["visits"] and meta["images"]["a"]["visits"] % 2048
    assert np.array_equal(z["a_sp_arr"], np.linspace(0, 190, 9, dtype=np.uint16)) and set(np.diff(z["a_sp_arr"].astype(int))) == {23, 24}


def test_sample_ref_err_is_capped(gold):
    """The restatement's distance from the 40-digit chain on the samples is below 64 eps / (0.07 arcsec) = 4.2e-8 output pixel, and not
    degenerate: 10 ref_err bounds the device in tests/test_gpu_inpool.py."""
    z, meta = gold
    for name in "ab":
        assert np.all(z[f"{name}_ref_err"] < 4.2e-8) and np.all(z[f"{name}_ref_err"] > 1e-11) and 100 <= len(z[f"{name}_sample_in"]) <= 2000


def test_image_d_has_only_border_nodes_in_range(gold):
    z, meta = gold
    lo, hi = P.limits(meta["n2"], meta["n1P"])
    x, y = z["d_nodes"]
    inr = (lo < x) & (x < hi) & (lo < y) & (y < hi)
    assert inr.any() and not inr[1:-1, 1:-1].any() and not z["d_relevant"].any()


def test_restatement_of_the_relevance_loop_equals_the_golden(gold):
    z, meta = gold
    for name, info in meta["images"].items():
        rel, mat = P.relevance(z[f"{name}_nodes"], z["use_instamps"], meta["n2"], meta["n1P"])
        assert rel == info["is_relevant"] and np.array_equal(mat, z[f"{name}_relevant"]), name


def test_host_loop_of_relevant_cells_equals_the_golden(gold):
    from pyimcom_amd import inpool

    z, meta = gold
    for name, info in meta["images"].items():
        rel, mat = inpool._relevance(z[f"{name}_nodes"], z["use_instamps"], meta["n2"], meta["n1P"])
        assert rel == info["is_relevant"] and mat.dtype == bool and np.array_equal(mat, z[f"{name}_relevant"]), name
    rb = z["b_relevant"]
    assert rb[0].any() and rb[:, 0].any() and not rb.all()  # two frame edges, and holes


def test_npixmax_of_equals_the_reference(gold):
    from pyimcom_amd import inpool

    z, meta = gold
    for name, info in meta["images"].items():
        if info["is_relevant"]:
            assert inpool.npixmax_of(meta["n2"], meta["dtheta_deg"]) == info["npixmax"]
    assert inpool.npixmax_of(32, 0.0390625 / 3600) == int(((32 * 0.0390625) / ((0.11 * 4.84813681109536e-06) / 4.84813681109536e-06) + 1) ** 2 * 1.05)


def test_restatement_of_the_partition_equals_the_golden(gold):
    z, meta = gold
    n = 0
    for name, key, info, masked in variants(meta):
        px, py = positions(z, name, meta["nside"])
        got = P.partition(px, py, z[f"{name}_relevant"], z[f"{name}_sp_arr"], z[f"{name}_mask"] if masked else None, z["use_instamps"], meta["n2"], meta["n1P"],
                          info["npixmax"])
        for k, v in zip(("y_idx", "x_idx", "y_val", "x_val", "pix_count"), got):
            assert v.dtype == z[f"{key}_{k}"].dtype and np.array_equal(v, z[f"{key}_{k}"]), (key, k)
        assert len(P.visits(z[f"{name}_relevant"], z[f"{name}_sp_arr"])[0]) == info["visits"]
        n += 1
    assert n == 6
    # the mask blanks stamp (5, 2) entirely, and single pixels elsewhere
    assert z["a_pix_count"][5, 2] == 0 < z["a_nomask_pix_count"][5, 2] and 0 < z["a_pix_count"].sum() < z["a_nomask_pix_count"].sum() - z["a_nomask_pix_count"][5, 2]
    # the hole and the unused border of use_instamps stay empty
    assert z["a_nomask_pix_count"][3, 4] == 0 and not z["a_nomask_pix_count"][0].any() and not z["a_nomask_pix_count"][:, 7].any()


def test_restatement_overflows_one_below_the_fullest_stamp(gold):
    z, meta = gold
    px, py = positions(z, "a", meta["nside"])
    full = int(z["a_nomask_pix_count"].max())
    args = (px, py, z["a_relevant"], z["a_sp_arr"], None, z["use_instamps"], meta["n2"], meta["n1P"])
    assert P.partition(*args, full)[4].max() == full
    with pytest.raises(P.Overflow):
        P.partition(*args, full - 1)


def test_restatement_of_extract_layers_equals_the_golden(gold):
    z, meta = gold
    for name, key, info, masked in variants(meta):
        for nf, dk in ((meta["n_inframe"], "data"), (1, "data1")):
            got = P.extract_layers(P.frames(nf, meta["nside"], info["no"]), z[f"{key}_y_idx"], z[f"{key}_x_idx"], z[f"{key}_pix_count"])
            assert got.dtype == np.float32 and got.shape == z[f"{key}_{dk}"].shape and np.array_equal(got, z[f"{key}_{dk}"]), (key, dk)


def test_restatement_of_the_instamps_equals_the_golden(gold):
    z, meta = gold
    images = [{k: z[f"{name}_{k}"] for k in ("y_val", "x_val", "data", "pix_count")} for name in meta["pool"] if meta["images"][name]["is_relevant"]]
    assert len(images) == 3
    stamps, cum = P.instamps(images, meta["n_inframe"])
    assert cum.dtype == np.uint32 and np.array_equal(cum, z["pool_pix_cumsum"])
    for got, k in zip(P.pool_arrays(stamps), ("pool_x", "pool_y", "pool_data", "pool_expo", "pool_inst_off")):
        assert got.dtype == z[k].dtype and np.array_equal(got, z[k]), k
    assert set(z["pool_expo"].tolist()) == {0, 1, 2}
    per_image = np.diff(z["pool_pix_cumsum"].astype(np.int64), axis=1)
    assert ((per_image == 0).any(axis=1) & (per_image > 0).any(axis=1)).any()  # stamps that some images leave empty


def test_visit_decode_against_plain_loops_under_sanitizers(tmp_path):
    exe = tmp_path / "partition_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "partition_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["ragged_190_8", "ragged_190_24", "all_190_8", "sca_4088_90", "empty_cells_5_8", "single_cell", "sparse_1000_90"]
    assert all(int(r[2]) == 0 for r in rows), rows
    checked = {r[0]: int(r[1]) for r in rows}
    assert checked["all_190_8"] == 190 * 190 and checked["empty_cells_5_8"] == 25 and checked["single_cell"] == 37 * 37 and checked["sparse_1000_90"] == 0
    assert checked["sca_4088_90"] > 10 ** 7
