"""pyimcom_amd.simmask on the device (csrc/pcg64.hip): draws against numpy's own generator, masks against the reference's outputs
(tests/golden/crmask.npz) and against the three lines of ``Mask.randmask`` restated with numpy at small sizes.  Every comparison is exact
equality: the device works in integers until the one exact conversion to a double, so there is no tolerance to choose."""

import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import crmask_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "crmask.npz"))
NSIDE = int(G["nside"])
SEEDS = (100000000 + 1234, 100000000 + 7, 5)
COUNTS = (0, 1, 63, 64, 65, 4097)  # a thread forms 8 draws, a workgroup 2048
OFFSETS = (0, 1, 2**32 - 3, 2**32 + 5, 2**64 - 2, 2**100 + 1)
DEV = "cuda:0"


def _numpy_draws(seed, offset, count):
    bg = np.random.PCG64(seed)
    bg.advance(offset)
    return np.random.Generator(bg).uniform(size=count)


def _numpy_randmask(idsca, pcut, nside, pad=10):
    """layer.py:954-964 with numpy alone: g = default_rng(100000000 + obs).uniform(size=(18, W, W))[sca - 1], W = nside + 2 pad; a pixel is
    good when no g < pcut lies in the 3 x 3 around it."""
    W = nside + 2 * pad
    hit = np.random.default_rng(100000000 + idsca[0]).uniform(size=(18, W, W))[idsca[1] - 1] < pcut
    near = np.zeros((nside, nside), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= hit[pad + dy:pad + dy + nside, pad + dx:pad + dx + nside]
    return ~near


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


@pytest.mark.parametrize("device", [None, DEV])
def test_uniform_equals_numpy(device):
    from pyimcom_amd import simmask

    for seed in SEEDS:
        for offset in OFFSETS:
            want = _numpy_draws(seed, offset, max(COUNTS))
            for count in COUNTS:
                got = simmask.uniform(seed, offset, count, device=device)
                assert (device is None) == isinstance(got, np.ndarray) and tuple(got.shape) == (count,)
                assert np.array_equal(_host(got), want[:count]), (seed, offset, count)
    bg = np.random.PCG64(SEEDS[0])  # a bit generator as it stands, and a shape
    bg.advance(12345)
    got = _host(simmask.uniform(bg, 3, (3, 5, 7), device=device))
    assert np.array_equal(got, _numpy_draws(SEEDS[0], 12348, 105).reshape(3, 5, 7))
    assert bg.state["state"]["state"] == R.jump(*R.stream(SEEDS[0]), 12345)  # left where it stood


def test_uniform_meets_rotation_zero():
    """The first 4097 draws of the first seed include rotations 0 and 63 (the rotate must not shift by 64)."""
    state, inc = R.stream(SEEDS[0])
    rots, s = set(), state
    for _ in range(4097):
        s = (R.MULT * s + inc) & R.M128
        rots.add(s >> 122)
    assert rots == set(range(64))


@pytest.mark.parametrize("device", [None, DEV])
def test_uniform_at(device):
    from pyimcom_amd import simmask

    pos = np.array([2**32 + 5, 0, 2**32 - 3, 1, 2**32 - 1, 2**32, 2**62 + 3, 65, 64, 63, 2**63 - 1, 2047, 2048], dtype=np.int64)
    for seed in SEEDS:
        got = _host(simmask.uniform_at(seed, pos, device=device))
        assert np.array_equal(got, np.array([_numpy_draws(seed, int(p), 1)[0] for p in pos])), seed
        for offset in OFFSETS[:-2]:
            perm = np.random.default_rng(1).permutation(300)
            run = _host(simmask.uniform(seed, offset, 300, device=device))
            assert np.array_equal(_host(simmask.uniform_at(seed, offset + perm.astype(np.int64), device=device)), run[perm])
        for offset in OFFSETS[-2:]:  # past int64: through the state
            bg = np.random.PCG64(seed)
            bg.advance(offset - 7)
            got = _host(simmask.uniform_at(bg, np.array([[9, 7], [8, 306]]), device=device))
            assert np.array_equal(got, _numpy_draws(seed, offset, 300)[[[2, 0], [1, 299]]])
    assert simmask.uniform_at(5, np.zeros((0,), dtype=np.int64), device=device).shape == (0,)
    with pytest.raises(ValueError):
        simmask.uniform_at(5, np.array([3, -1]))


@pytest.mark.parametrize("case", range(len(G["mask_pcut"])))
def test_randmask_golden(case):
    from pyimcom_amd import simmask

    idsca, pcut = tuple(int(v) for v in G["mask_idsca"][case]), float(G["mask_pcut"][case])
    got = simmask.randmask(idsca, pcut, nside=NSIDE)
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, G["masks"][case])
    dev = simmask.randmask(idsca, pcut, nside=NSIDE, device_out=True)
    assert dev.is_cuda and str(dev.dtype) == "torch.uint8" and dev.cpu().numpy().tobytes() == got.tobytes()
    assert simmask.randmask(idsca, pcut, hitinfo={}) is None  # layer.py:961


@pytest.mark.parametrize("nside", [1, 2, 61, 64, 65])
def test_randmask_sizes_slices_and_count(nside):
    """Sides around the tile (62 x 30 outputs a workgroup) and the 8-pixel runs; the first and the last slice; no hit and all hits."""
    from pyimcom_amd import simmask

    for sca in (1, 18):
        for pcut in (0.0, 0.05, 1.0):
            want = _numpy_randmask((7, sca), pcut, nside)
            assert np.array_equal(simmask.randmask((7, sca), pcut, nside=nside), want), (sca, pcut)
            mask, ngood = simmask.cr_mask(100000007, nside, sca - 1, pcut)
            assert mask.dtype == np.uint8 and ngood == np.count_nonzero(mask) == np.count_nonzero(want)
            assert (pcut != 0.0 or want.all()) and (pcut != 1.0 or not want.any())


def test_randmask_full_size_digest():
    from pyimcom_amd import simmask

    nside, obs, sca = (int(v) for v in G["full_pars"])
    pcut = float(G["full_pcut"])
    got = simmask.randmask((obs, sca), pcut, nside=nside)
    assert got.shape == (nside, nside)
    assert np.array_equal(np.count_nonzero(got, axis=1).astype(np.int32), G["full_row_counts"])
    assert np.count_nonzero(got) == int(G["full_total"])
    assert np.array_equal(got[G["full_rows_idx"]], G["full_rows"])
    dev, ngood = simmask.cr_mask(100000000 + obs, nside, sca - 1, pcut, device=DEV)  # run to run, device out, the count
    assert ngood == int(G["full_total"]) and dev.cpu().numpy().tobytes() == got.tobytes()


def _inimage(lab, rate, thr, idsca):
    cfg = types.SimpleNamespace(cr_mask_rate=rate, extrainput=[None, "labnoise"], labnoisethreshold=thr)
    return types.SimpleNamespace(blk=types.SimpleNamespace(cfg=cfg), idsca=idsca, indata=[None, lab])


def test_load_cr_mask(capsys):
    import torch

    from pyimcom_amd import simmask

    rate, thr = (float(v) for v in G["lab_pars"])
    lab, idsca = G["lab_layer"], tuple(int(v) for v in G["lab_idsca"])
    got = simmask.load_cr_mask(_inimage(lab, rate, thr, idsca))
    assert got.dtype == np.bool_ and np.array_equal(got, G["lab_mask"])
    assert not got[3, 4] and not got[10, 0]  # the NaN; float32(0.7) against the Python float 0.7, compared in float32
    assert f"good pix -->  {np.count_nonzero(got)} /" in capsys.readouterr().out
    assert np.array_equal(simmask.load_cr_mask(_inimage(torch.as_tensor(lab, device=DEV), rate, thr, idsca)), got)
    wide = simmask.load_cr_mask(_inimage(lab, rate, np.float64(thr), idsca))  # a float64 scalar: numpy compares in float64
    assert np.array_equal(wide, np.logical_and(_numpy_randmask(idsca, rate, NSIDE), np.abs(lab) < np.float64(thr)))
    assert simmask.load_cr_mask(_inimage(lab, 0.0, thr, idsca)) is None
    plain = types.SimpleNamespace(blk=types.SimpleNamespace(cfg=types.SimpleNamespace(cr_mask_rate=rate, extrainput=[None])), idsca=idsca)
    m = simmask.load_cr_mask(plain)  # no lab noise: the mask of the full chip side
    assert m.shape == (simmask._sca_nside(),) * 2 and m.dtype == np.bool_


@pytest.mark.parametrize("key", ["sub", "big"])
def test_subgen_golden(key):
    from pyimcom_amd import simmask

    seed, P, lenpix = (int(v) for v in G[f"{key}_pars"])
    pix = G[f"{key}_pix"]
    want = np.random.PCG64(seed)
    want.advance(P * lenpix)
    bg = np.random.PCG64(seed)
    got = simmask.subgen_multirow(bg, lenpix, pix, P)
    assert got.shape == (P, pix.size) and np.array_equal(got, G[f"{key}_out"])
    assert bg.state == want.state
    assert [bg.state["state"]["state"] & R.M64, bg.state["state"]["state"] >> 64] == [int(v) for v in G[f"{key}_state_after"]]
    bg = np.random.PCG64(seed)
    rows = [simmask.subgen(bg, lenpix, pix) for _ in range(P)]  # row by row from the moving generator
    assert np.array_equal(np.stack(rows), G[f"{key}_out"]) and bg.state == want.state
    bg = np.random.PCG64(seed)
    empty = simmask.subgen(bg, lenpix, np.zeros(0, dtype=np.int64))
    assert empty.shape == (0,) and empty.dtype == np.float64
    one = np.random.PCG64(seed)
    one.advance(lenpix)
    assert bg.state == one.state
    assert np.array_equal(simmask.subgen(bg, lenpix, pix), G[f"{key}_out"][1])  # the empty call moved the stream by one row


def test_subgen_rows_past_int64():
    from pyimcom_amd import simmask

    bg, lenpix = np.random.PCG64(9), 2**62
    got = simmask.subgen_multirow(bg, lenpix, np.array([3, 0]), 3)
    assert np.array_equal(got, np.array([[_numpy_draws(9, j * lenpix + p, 1)[0] for p in (3, 0)] for j in range(3)]))
    want = np.random.PCG64(9)
    want.advance(3 * lenpix)
    assert bg.state == want.state


def test_refusals():
    from pyimcom_amd import _lib, simmask

    for bad in (np.random.MT19937(1), np.random.Philox(1), np.random.SFC64(1), "seed"):
        with pytest.raises(TypeError):
            simmask.uniform(bad, 0, 4)
        with pytest.raises(TypeError):
            simmask.uniform_at(bad, np.array([1]))
    with pytest.raises(TypeError):
        simmask.subgen(np.random.MT19937(1), 10, np.array([1]))
    with pytest.raises(TypeError):
        simmask.cr_mask(1, 4, 0, 0.1, labnoise=np.zeros((4, 4)))  # float64 lab noise would compare differently
    ctx = _lib.default_context()
    mask, ngood, out = np.zeros((4, 4), dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(4)
    u = C.c_uint64

    def cr(nside=4, pad=10, sl=0, n_slices=18):
        return _lib.lib.imcom_cr_mask(ctx.handle, u(1), u(0), u(1), u(0), nside, pad, sl, n_slices, 0.5, None, 0.0, _lib.ptr(mask), _lib.ptr(ngood), _lib.MEM_HOST)

    assert cr() == 0
    for kw in ({"pad": 0}, {"sl": 18}, {"sl": -1}, {"nside": 0}, {"n_slices": 0}, {"pad": -3}):
        assert cr(**kw) == -1, kw  # IMCOM_ERR_ARG
        assert "cr_mask" in _lib.lib.imcom_last_error().decode()
    assert _lib.lib.imcom_pcg64_uniform(ctx.handle, u(1), u(0), u(1), u(0), u(0), u(0), -1, _lib.ptr(out), _lib.MEM_HOST) == -1
    assert _lib.lib.imcom_pcg64_uniform_at(ctx.handle, u(1), u(0), u(1), u(0), None, -1, _lib.ptr(out), _lib.MEM_HOST) == -1
    assert _lib.lib.imcom_pcg64_uniform(ctx.handle, u(1), u(0), u(1), u(0), u(0), u(0), 4, None, _lib.MEM_HOST) == -1
    with pytest.raises(_lib.ImcomError):
        simmask.cr_mask(1, 4, 18, 0.1)


def test_run_to_run():
    from pyimcom_amd import simmask

    a, b = simmask.uniform(SEEDS[0], 2**64 - 2, 4097), simmask.uniform(SEEDS[0], 2**64 - 2, 4097)
    assert a.tobytes() == b.tobytes()
    a, b = simmask.randmask((1234, 18), 0.05, nside=65), simmask.randmask((1234, 18), 0.05, nside=65)
    assert a.tobytes() == b.tobytes()
