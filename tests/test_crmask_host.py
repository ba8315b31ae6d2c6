"""CPU-side checks of the PCG64 draws and the cosmic-ray mask (pyimcom_amd/simmask.py, csrc/pcg64.hip): the plain-integer restatement
(tests/crmask_reference.py) against numpy's own ``Generator.uniform`` and against the reference's outputs (tests/golden/crmask.npz), and
the golden against a fresh run of the reference where its tree is present.  Every comparison is exact equality: the quantities are
integers, booleans, or doubles formed by one exact conversion.  No GPU.

The restatement walks the stream in Python ints, about a microsecond a draw: of the full-size digest it forms the four stored rows, and
the good-pixel counts of ROWS_SAMPLED rows; the device test (tests/test_gpu_crmask.py) checks all 4088 counts and the total."""

import importlib.util
import os

import numpy as np
import pytest

from tests import crmask_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "crmask.npz"))
NSIDE = int(G["nside"])
ROWS_SAMPLED = (0, 1, 2, 511, 2043, 2044, 3000, 4085, 4086, 4087)
REFERENCE = "/root/reference/src/pyimcom/layer.py"


@pytest.mark.parametrize("seed", [0, 1, 100001234, 100000007, 2**63 + 11])
def test_restatement_equals_numpy(seed):
    state, inc = R.stream(seed)
    for offset in (0, 1, 2**32 - 3, 2**32 + 5, 2**64 - 2, 2**100 + 1):
        bg = np.random.PCG64(seed)
        bg.advance(offset)
        want = np.random.Generator(bg).uniform(size=67)
        assert np.array_equal(np.array(R.uniform(state, inc, offset, 67)), want), (seed, offset)
        assert [R.uniform_at(state, inc, offset + k) for k in (0, 66)] == [want[0], want[66]]
    assert np.array_equal(np.array(R.uniform(state, inc, 0, 300)), np.random.default_rng(seed).uniform(size=300))  # default_rng is PCG64(seed)


def test_restatement_meets_rotation_zero():
    """Among the first 300 draws of a seed some have the rotation s >> 122 = 0 (one in 64): the shift by 64 that a careless rotate makes."""
    state, inc = R.stream(100001234)
    s, rots = state, []
    for _ in range(300):
        s = (R.MULT * s + inc) & R.M128
        rots.append(s >> 122)
    assert 0 in rots and 63 in rots


def test_slice_of_the_padded_draw():
    """layer.py:957: slice s of uniform(size=(18, W, W)) is draws s W^2 .. (s + 1) W^2 - 1, row-major."""
    n, seed = 9, 100000007
    W = n + 2 * R.PAD
    g = np.random.default_rng(seed).uniform(size=(R.N_SLICES, W, W))
    state, inc = R.stream(seed)
    for s, r, c in ((0, 0, 0), (17, W - 1, W - 1), (8, 11, 3)):
        assert R.uniform_at(state, inc, s * W * W + r * W + c) == g[s, r, c]


@pytest.mark.parametrize("case", range(len(G["mask_pcut"])))
def test_restatement_reproduces_the_golden_masks(case):
    idsca, pcut = G["mask_idsca"][case], float(G["mask_pcut"][case])
    got = R.randmask(idsca, pcut, NSIDE)
    assert got.dtype == bool and np.array_equal(got, G["masks"][case])
    assert 0 < np.count_nonzero(got) < got.size  # the case has hits and good pixels


def test_restatement_reproduces_the_golden_labnoise_case():
    rate, thr = G["lab_pars"]
    lab = G["lab_layer"]
    assert lab.dtype == np.float32 and np.isnan(lab).sum() == 1 and (np.abs(lab) < np.float32(thr)).any() and (np.abs(lab) > np.float32(thr)).any()
    want = np.logical_and(R.randmask(G["lab_idsca"], float(rate), NSIDE), np.abs(lab) < float(thr))
    assert np.array_equal(want, G["lab_mask"])
    assert not G["lab_mask"][3, 4] and not G["lab_mask"][10, 0]  # the NaN; float32(0.7) is not below 0.7 compared in float32


@pytest.mark.parametrize("key", ["sub", "big"])
def test_restatement_reproduces_the_golden_subgen(key):
    seed, P, lenpix = (int(v) for v in G[f"{key}_pars"])
    state, inc = R.stream(seed)
    out, after = R.subgen_multirow(state, inc, lenpix, G[f"{key}_pix"], P)
    assert np.array_equal(out, G[f"{key}_out"])
    assert [after & R.M64, after >> 64] == [int(v) for v in G[f"{key}_state_after"]]
    bg = np.random.PCG64(seed)
    bg.advance(P * lenpix)
    assert bg.state["state"]["state"] == after


def test_restatement_reproduces_the_full_size_digest():
    nside, obs, sca = (int(v) for v in G["full_pars"])
    pcut = float(G["full_pcut"])
    rows = [int(r) for r in G["full_rows_idx"]]
    assert np.array_equal(R.mask_rows(R.SEED0 + obs, nside, sca - 1, pcut, rows), G["full_rows"])
    got = R.mask_rows(R.SEED0 + obs, nside, sca - 1, pcut, list(ROWS_SAMPLED))
    assert np.array_equal(np.count_nonzero(got, axis=1), G["full_row_counts"][list(ROWS_SAMPLED)])
    assert int(G["full_total"]) == int(G["full_row_counts"].astype(np.int64).sum()) and G["full_row_counts"].shape == (nside,)


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference tree is not on this machine")
def test_golden_regenerates_bit_for_bit():
    spec = importlib.util.spec_from_file_location("make_golden_crmask", os.path.join(ROOT, "tests", "golden", "make_golden_crmask.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.main(full=True, save=False)
    assert sorted(fresh) == sorted(G.files)
    for k in G.files:
        assert fresh[k].dtype == G[k].dtype and np.array_equal(fresh[k], G[k], equal_nan=G[k].dtype.kind == "f"), k


def test_python_layer_refusals_and_host_logic():
    """What pyimcom_amd.simmask decides on the host, before any device call."""
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import _dev, simmask

    with pytest.raises(TypeError):
        simmask.uniform(np.random.MT19937(1), 0, 4)
    with pytest.raises(TypeError):
        simmask.subgen(np.random.Philox(1), 10, np.array([1]))
    with pytest.raises(ValueError):
        simmask.uniform(1, -1, 4)
    assert simmask._stream(np.random.default_rng(5)) == R.stream(5)
    assert _dev.compare_value(0.7, np.float32) == float(np.float32(0.7)) and _dev.compare_value(np.float64(0.7), np.float32) == 0.7
    bg = np.random.PCG64(3)
    assert simmask.subgen(bg, 2**31 + 7, np.zeros(0, dtype=np.int64)).shape == (0,)  # empty: nothing is drawn, the stream still moves
    want = np.random.PCG64(3)
    want.advance(2**31 + 7)
    assert bg.state == want.state
    cfg = type("Cfg", (), {"cr_mask_rate": 0.0, "extrainput": [None]})()
    assert simmask.load_cr_mask(type("In", (), {"blk": type("Blk", (), {"cfg": cfg})(), "idsca": (1, 1)})()) is None
