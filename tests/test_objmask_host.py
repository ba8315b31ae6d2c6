"""The numpy restatement of the bright-object mask (tests/objmask_reference.py) against the reference's own outputs, recorded in
tests/golden/objmask.npz by tests/golden/make_golden_objmask.py: every case, every intermediate, bit for bit.  Also the host-compilable
core of the kernels (csrc/objmask_core.h) against the standard library (tests/native/objmask_check.cpp).  No device is touched."""

import os
import subprocess

import numpy as np
import pytest

from tests import objmask_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "objmask.npz"))
CASES = [str(c) for c in G["cases"]]
SCALARS = ("median_val", "bkg", "mad", "sigma", "seed_threshold", "grow_threshold")
MASKS = ("high_value_mask", "seed_mask", "grow_candidates", "grown_mask")


def same(a, b):
    """Equal values and equal types (NaN equals NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def edge_inputs(dtype):
    """Arrays on which a median can go wrong: ties across the middle, values one ulp apart, signed zeros, infinities, a NaN."""
    rng = np.random.default_rng(2)
    one = dtype(1)
    out = {}
    for n in (1, 2, 3, 255, 256, 257, 65537):
        x = rng.standard_normal(n)
        out[f"levels_{n}"] = (np.clip(np.round(x * 1.5), -3, 3) / 4).astype(dtype)  # 7 levels: whole buckets tie
        out[f"ulps_{n}"] = np.nextafter(one, dtype(2)) + np.spacing(one) * rng.integers(0, 9, size=n).astype(dtype)
        z = x.astype(dtype)
        z[:: 3] = np.where(rng.uniform(size=z[::3].size) < 0.5, dtype(0.0), dtype(-0.0))
        out[f"zeros_{n}"] = z
        w = x.astype(dtype)
        w[:: 4] = np.inf
        w[1:: 4] = -np.inf
        out[f"inf_{n}"] = w
        v = x.astype(dtype)
        v[n // 2] = np.nan
        out[f"nan_{n}"] = v
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_reference_bit_for_bit(name):
    image, (m, c), kind = G[f"{name}__image"], G[f"{name}__pars"], str(G[f"{name}__type"])
    m = int(m) if m == int(m) else float(m)  # the generator passed Python numbers
    d = {}
    out, mask = R.apply_object_mask(image.copy(), threshold_m=m, threshold_c=float(c), type=kind, details=d)
    assert mask.dtype == np.bool_ and np.array_equal(mask, G[f"{name}__neighbor_mask"])
    assert same(out, G[f"{name}__image_out"])
    seen = 0
    for q in SCALARS + MASKS:
        if f"{name}__{q}" in G.files:
            assert same(d[q], G[f"{name}__{q}"]), q
            seen += 1
    assert seen >= (2 if kind != "jwst" else 3)
    inpl = image.copy()
    out2, mask2 = R.apply_object_mask(inpl, threshold_m=m, threshold_c=float(c), inplace=True, type=kind)
    assert out2 is inpl and same(inpl, G[f"{name}__image_out"]) and np.array_equal(mask2, mask)
    out3, mask3 = R.apply_object_mask(image.copy(), mask=mask, type=kind)  # a given mask is applied as it is
    assert mask3 is mask and same(out3, out)


def test_the_cases_take_the_branches_they_are_there_for():
    assert G["jwst_const__mad"] == 0 and G["jwst_const__sigma"] == 0 and not G["jwst_const__neighbor_mask"].any()
    assert not G["jwst_nonfinite__neighbor_mask"].any() and not np.isfinite(G["jwst_nonfinite__image"]).any()
    assert G["jwst_f32__sigma"].dtype == np.float32 and G["jwst_f32__seed_threshold"] > 0.05  # 6 sigma above threshold_c
    assert G["jwst_f64__seed_threshold"] == 0.3  # threshold_c above 6 sigma
    img = G["fits_m0__image"]
    thr = np.float32(0.3)
    on = np.argwhere(img == thr)
    assert len(on) >= 1 and all(G["fits_m0__high_value_mask"][y, x] for y, x in on)
    below = np.argwhere(img == np.nextafter(thr, np.float32(0)))
    assert len(below) >= 1 and not any(G["fits_m0__high_value_mask"][y, x] for y, x in below)
    edge = G["fits_m0__neighbor_mask"]
    assert edge[0].any() and edge[-1].any() and edge[:, -1].any()  # sources on the borders


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_median_of_the_restatement_is_numpys(dtype):
    for name, a in edge_inputs(dtype).items():
        with np.errstate(invalid="ignore"):
            want = np.median(a)
        assert same(R.median(a), want), name


def test_dilation_and_propagation_of_the_restatement_are_scipys():
    for name in ("corners", "edges_tiles", "row"):
        for r in (1, 2, 4):
            assert np.array_equal(R.dilate(G[f"dil_{name}"], r), G[f"dil_{name}_r{r}"]), (name, r)
        assert np.array_equal(R.dilate(R.dilate(G[f"dil_{name}"], 2), 2), G[f"dil_{name}_r4"])
    got = R.propagate(G["prop_seed"], G["prop_grow"])
    assert np.array_equal(got, G["prop_out"])
    assert got[35, 35] and got[35, 36] and not got[21, 21] and not got[10:14, 10:14].any() and got[29, 5]


def test_native_core_against_the_standard_library(tmp_path):
    exe = tmp_path / "objmask_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "pyimcom_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "objmask_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[:2] for r in rows] == [["select", "float32"], ["select", "float64"], ["flood", "tile"]]
    assert all(int(r[2]) > 0 and int(r[3]) == 0 for r in rows), rows
