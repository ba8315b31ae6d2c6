"""Noise power spectra on the device (pyimcom_amd/noisespec.py, csrc/noisespec.hip) against the golden vectors of the reference's own lines
and, for sides too large to commit, the numpy restatement.  The bound of every quantity is max(10 |float64 numpy run - extended|,
2e-13 max|extended|), both terms from the fixture (tests/noisespec_reference.py:bound); the device must also be at least as close to the
extended evaluation as the reference's own (complex64) output is."""

import os
import types

import numpy as np
import pytest

from tests import noisespec_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "noisespec.npz"))
BDPAD = int(G["bdpad"])


@pytest.fixture(scope="module")
def ns():
    from pyimcom_amd import noisespec

    return noisespec


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _close(name, got, f64, ext, scale=None, ref=None):
    got = _np(got)
    obs = np.abs(got - ext).max()
    b = R.bound(np.abs(f64 - ext).max(), np.abs(ext).max() if scale is None else scale)
    print(f"{name}: observed {obs:.3e} bound {b:.3e}" + ("" if ref is None else f" reference's own {np.abs(ref - ext).max():.3e}"))
    assert obs <= b, (name, obs, b)
    if ref is not None:
        assert obs <= np.abs(ref - ext).max(), (name, obs, np.abs(ref - ext).max())


@pytest.mark.parametrize("side", [int(s) for s in G["anal_sides"]])
def test_noise_anal_call_against_golden(ns, side):
    """noise_anal_call on a duck-typed NoiseAnal (host float32 block, the crop by n2 * postage_pad and to Lcut): 52 -> 48 on the butterflies,
    56, 88, 104 on two-level lines with odd N2."""
    k = f"anal{side}"
    cfg = types.SimpleNamespace(NsideP=side + 2 * BDPAD, Nside=side, n2=2, postage_pad=BDPAD // 2, dtheta=float(G["dtheta"]), use_filter=2)
    obj = types.SimpleNamespace(cfg=cfg, layer="whitenoise1", outim=types.SimpleNamespace(get_coadded_layer=lambda layer: G[f"{k}_in"]))
    ns.noise_anal_call(obj, padding=False)
    Lcut = side // 8 * 8
    assert ns.route(Lcut) == (ns.ROUTE_LINES if side == 52 else ns.ROUTE_TWOLEVEL)
    assert obj.ps2d.shape == (Lcut // 8, Lcut // 8) and obj.ps1d.shape == (Lcut // 16, 2) and obj.ps2d.dtype == np.float64
    _close(f"{k} ps2d", obj.ps2d, G[f"{k}_ps2d_f64"], G[f"{k}_ps2d_ext"], ref=G[f"{k}_ps2d_ref"])
    mext = G[f"{k}_ps1d_ext"]
    _close(f"{k} mean", obj.ps1d[:, 0], G[f"{k}_ps1d_f64"][:, 0], mext[:, 0], ref=G[f"{k}_ps1d_ref"][:, 0])
    _close(f"{k} err", obj.ps1d[:, 1], G[f"{k}_ps1d_f64"][:, 1], mext[:, 1], scale=np.abs(mext[:, 0]).max(), ref=G[f"{k}_ps1d_ref"][:, 1])
    assert obj.ps1d[-1, 1] == 0.0


@pytest.mark.parametrize("key", ["report56b", "report48b", "report48u"])
def test_windowed_report_against_golden(ns, key):
    """NoiseReport.measure_power_spectrum with the window, from a float32 tensor on the device; bin8 off at side 48."""
    import torch

    w, bin8 = G[f"{key}_window"], key.endswith("b")
    a = torch.as_tensor(G[f"{key}_in"], device="cuda:0")
    ps = ns.power_spectrum_2d(a, ns.windowed_norm(float(G[f"{key}_norm"]), w), w, bin8)
    assert ps.is_cuda and ps.dtype == torch.float64
    assert np.array_equal(G[f"{key}_ps2d_ref"], G[f"{key}_ps2d_f64"])  # (frame * window is float64: the reference's own run is the float64 run)
    _close(key, ps, G[f"{key}_ps2d_f64"], G[f"{key}_ps2d_ext"])
    if bin8:
        side = a.shape[0]
        mean, err = ns.azimuthal_average(ps, side // 16)
        e = G[f"{key}_ps1d_ext"]
        _close(f"{key} mean", mean, G[f"{key}_ps1d_f64"][:, 0], e[:, 0])
        _close(f"{key} err", err, G[f"{key}_ps1d_f64"][:, 1], e[:, 1], scale=np.abs(e[:, 0]).max())
        assert float(err[-1]) == 0.0


@pytest.fixture(scope="module")
def frames56():
    rng = np.random.default_rng(56)
    return rng.standard_normal((3, 56, 56)).astype(np.float32)


def test_a_frame_gives_the_same_bits_alone_in_a_batch_and_again(ns, frames56):
    import torch

    t = torch.as_tensor(frames56, device="cuda:0")
    norms = np.array([1.0, 2.0, 3.0])
    three = ns.power_spectrum_2d(t, norms)
    assert torch.equal(three, ns.power_spectrum_2d(t, norms))
    for f in range(3):
        assert torch.equal(three[f], ns.power_spectrum_2d(t[f], norms[f]))
    assert torch.equal(three[:2], ns.power_spectrum_2d(t[:2], norms[:2]))
    assert torch.equal(three, ns.power_spectrum_2d(t, norms, frames_per_call=2))
    assert np.array_equal(three.cpu().numpy(), ns.power_spectrum_2d(frames56, norms))  # host input
    for f in range(3):
        ext = R.power_spectrum_2d(frames56[f], norms[f], extended=True).astype(np.float64)
        _close(f"frame {f}", three[f], R.power_spectrum_2d(frames56[f], norms[f]), ext)


def test_float64_input_and_a_view_inside_a_padded_block(ns, frames56):
    import torch

    block = torch.zeros((3, 70, 72), dtype=torch.float64, device="cuda:0")
    block[:, 5:61, 9:65] = torch.as_tensor(frames56.astype(np.float64) + 1e-9, device="cuda:0")
    view = block[:, 5:61, 9:65]
    assert not view.is_contiguous()
    got = ns.power_spectrum_2d(view, 1.5)
    assert torch.equal(got, ns.power_spectrum_2d(view.contiguous(), 1.5))
    a = view[1].cpu().numpy()
    _close("float64 view", got[1], R.power_spectrum_2d(a, 1.5), R.power_spectrum_2d(a, 1.5, extended=True).astype(np.float64))
    v32 = block.to(torch.float32)[:, 5:61, 9:65]
    assert torch.equal(ns.power_spectrum_2d(v32, 1.5), ns.power_spectrum_2d(v32.contiguous(), 1.5))


def test_side_136_takes_the_dense_route(ns):
    assert ns.route(136) == ns.ROUTE_DENSE
    a = np.random.default_rng(136).standard_normal((2, 136, 136)).astype(np.float32)
    got = ns.power_spectrum_2d(a, 4.0)
    assert np.array_equal(got[1], ns.power_spectrum_2d(a[1], 4.0))
    for f in range(2):
        _close(f"136 frame {f}", got[f], R.power_spectrum_2d(a[f], 4.0), R.power_spectrum_2d(a[f], 4.0, extended=True).astype(np.float64))


@pytest.fixture(scope="module")
def case1040():
    a = np.random.default_rng(1040).standard_normal((1040, 1040)).astype(np.float32)
    norm = (1040 / 0.04) ** 2
    f64 = R.power_spectrum_2d(a, norm)
    ext = R.power_spectrum_2d(a, norm, extended=True)
    m64, e64 = R.azimuthal_average(f64, 65)
    mx, ex = R.azimuthal_average(ext, 65, extended=True)
    return a, norm, f64, ext.astype(np.float64), (m64, e64), (mx.astype(np.float64), ex.astype(np.float64))


@pytest.mark.parametrize("how", ["two-level", "dense", "switch"])
def test_side_1040_on_both_routes(ns, case1040, how, monkeypatch):
    """1040 = 80 x 13: two-level lines above 1024, and the dense route by argument and by IMCOM_NOISEPS_ROUTE=dense; each against the
    restatement's extended evaluation with the bound of the float64 numpy run."""
    a, norm, f64, ext, (m64, e64), (mx, ex) = case1040
    monkeypatch.delenv("IMCOM_NOISEPS_ROUTE", raising=False)
    if how == "switch":
        monkeypatch.setenv("IMCOM_NOISEPS_ROUTE", "dense")
    assert ns.route(1040) == (ns.ROUTE_DENSE if how == "switch" else ns.ROUTE_TWOLEVEL)
    got = ns.power_spectrum_2d(a, norm, route={"two-level": ns.ROUTE_TWOLEVEL, "dense": ns.ROUTE_DENSE, "switch": 0}[how])
    _close(f"1040 {how} ps2d", got, f64, ext)
    mean, err = ns.azimuthal_average(got, 65)
    _close(f"1040 {how} mean", mean, m64, mx)
    _close(f"1040 {how} err", err, e64, ex, scale=np.abs(mx).max())
    assert err[-1] == 0.0


def test_an_empty_annulus_is_nan_and_a_single_pixel_has_no_error(ns):
    img = np.random.default_rng(3).standard_normal((9, 9))
    rbin = R.radial_labels(9, 4)
    rbin[rbin == 2] = 1
    mean, err = ns.azimuthal_average(img, 4, rbin=rbin)
    assert np.isnan(mean[1]) and np.isnan(err[1]) and err[-1] == 0.0 and mean[-1] == img[0, 0]
    m, e = R.azimuthal_average(img, 4, rbin)
    ok = ~np.isnan(m)
    np.testing.assert_allclose(mean[ok], m[ok], rtol=1e-13)
    np.testing.assert_allclose(err[ok], e[ok], rtol=1e-12, atol=1e-15)


def test_noise_spectra_over_a_small_mosaic(ns):
    """NoiseSpectra over 2 x 2 blocks of side 56, two layers, two coverage bins, against the loop of analysis.py:1270-1303 in numpy."""
    import torch

    rng = np.random.default_rng(22)
    blocks = [[rng.standard_normal((2, 56, 56)).astype(np.float32) for _ in range(2)] for _ in range(2)]
    cov = np.array([[0, 1], [1, 1]])
    norm = (56 / 0.04) ** 2
    acc = ns.NoiseSpectra(56, 2, 2, norm=norm)
    for iby in range(2):  # (the device adds a block's layers together: per layer the blocks still arrive in the loop's order)
        for ibx in range(2):
            acc.add(torch.as_tensor(blocks[iby][ibx], device="cuda:0") if ibx else blocks[iby][ibx], cov[iby][ibx])
    ps2d, ps1d, wn = acc.result([1, 3], 4)
    want2d, want1d = R.mosaic(blocks, cov, 2, norm)
    assert ps2d.shape == (2, 7, 7) and ps1d.shape == (2, 2, 3, 2) and wn.shape == (3,)
    np.testing.assert_allclose(ps2d, want2d, rtol=0, atol=2e-13 * want2d.max())
    np.testing.assert_allclose(ps1d, want1d, rtol=0, atol=2e-13 * want1d.max())
    np.testing.assert_allclose(wn, R.wavenumbers(56, 3), rtol=1e-14)


def test_blockmaps_noise_spectrum_reads_the_block_in_place(ns):
    import torch

    from pyimcom_amd.block import BlockMaps

    bm = BlockMaps(8, 8, 2, 4, 1)  # side 64 + 2 x 2 of fade; pad 4 a side leaves 56
    bm._out_map.copy_(torch.as_tensor(np.random.default_rng(8).standard_normal(tuple(bm._out_map.shape)).astype(np.float32)))
    got = bm.noise_spectrum([1, 2], 4, [2.0, 3.0])
    crop = bm.out_map[0, 1:3, 6:62, 6:62].cpu().numpy()
    want = ns.power_spectrum_2d(crop, [2.0, 3.0])
    assert got.is_cuda and tuple(got.shape) == (2, 7, 7) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(bm.noise_spectrum([3, 1], 4, 1.0).cpu().numpy(), ns.power_spectrum_2d(bm.out_map[0, [3, 1], 6:62, 6:62].cpu().numpy(), 1.0))
