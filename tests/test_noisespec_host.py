"""CPU-side checks of the noise power spectra (pyimcom_amd/noisespec.py): the numpy restatement against the golden float64 run of the
reference's own lines, the fold of analysis.py:790-793, the labels, the route per side, refusals and the byte plan.  No GPU."""

import os

import numpy as np
import pytest

from tests import noisespec_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "noisespec.npz"))
BDPAD = int(G["bdpad"])


@pytest.fixture(scope="module")
def ns():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import noisespec

    return noisespec


def _close(name, got, f64, ext, scale=None):
    obs = np.abs(got - ext).max()
    b = R.bound(np.abs(f64 - ext).max(), np.abs(ext).max() if scale is None else scale)
    print(f"{name}: observed {obs:.3e} bound {b:.3e}")
    assert obs <= b, (name, obs, b)


@pytest.mark.parametrize("side", [int(s) for s in G["anal_sides"]])
def test_restatement_equals_the_golden_float64_run(side):
    k = f"anal{side}"
    ps2d, ps1d = R.noise_anal(G[f"{k}_in"].astype(np.float64), BDPAD, lambda L: float(G[f"{k}_norm"]))
    _close(f"{k} ps2d", ps2d, G[f"{k}_ps2d_f64"], G[f"{k}_ps2d_ext"])
    _close(f"{k} mean", ps1d[:, 0], G[f"{k}_ps1d_f64"][:, 0], G[f"{k}_ps1d_ext"][:, 0])
    _close(f"{k} err", ps1d[:, 1], G[f"{k}_ps1d_f64"][:, 1], G[f"{k}_ps1d_ext"][:, 1], scale=np.abs(G[f"{k}_ps1d_ext"][:, 0]).max())
    assert ps1d[-1, 1] == 0.0 and G[f"{k}_ps1d_f64"][-1, 1] == 0.0  # the outermost annulus is the corner pixel alone


@pytest.mark.parametrize("key", ["report56b", "report48b", "report48u"])
def test_restatement_equals_the_golden_report(key):
    w = G[f"{key}_window"]
    ps = R.power_spectrum_2d(G[f"{key}_in"], float(G[f"{key}_norm"]) * np.average(w**2), w, key.endswith("b"))
    _close(key, ps, G[f"{key}_ps2d_f64"], G[f"{key}_ps2d_ext"])


@pytest.mark.parametrize("L", [8, 48, 56])
def test_fold_of_rfft2_is_the_shifted_full_spectrum(L):
    a = np.random.default_rng(L).standard_normal((L, L))
    full = np.fft.fftshift(np.abs(np.fft.fft2(a)) ** 2) / 2.5
    np.testing.assert_allclose(R.fold_rfft2(a, 2.5), full, rtol=1e-12, atol=1e-12 * full.max())
    np.testing.assert_allclose(R.power_spectrum_2d(a, 2.5, None, False), full, rtol=1e-12, atol=1e-12 * full.max())


@pytest.mark.parametrize("n,nrad", [(6, 3), (7, 3), (13, 6), (320, 160)])
def test_radial_labels(ns, n, nrad):
    yy, xx = np.mgrid[:n, :n]  # analysis.py:691-695
    r = np.hypot(xx - n / 2, yy - n / 2)
    want = (nrad * r / r.max()).astype(int)
    got = ns.radial_labels(n, nrad)
    assert np.array_equal(got, want)
    L = 8 * n  # 1260-1262
    r = np.hypot(xx - L // 8 / 2, yy - L // 8 / 2)
    assert np.array_equal(got, (nrad * r / r.max()).astype(int))
    assert got.max() == nrad and (got == nrad).sum() == 1 and got[0, 0] == nrad


@pytest.mark.parametrize("side", [int(s) for s in G["anal_sides"]])
def test_wavenumbers(ns, side):
    L = side // 8 * 8
    _close(f"wavenumbers {L}", ns.wavenumbers(L, L // 16), G[f"anal{side}_wn_f64"], G[f"anal{side}_wn_ext"])


def test_routes(ns, monkeypatch):
    monkeypatch.delenv("IMCOM_NOISEPS_ROUTE", raising=False)
    want = {48: ns.ROUTE_LINES, 768: ns.ROUTE_LINES, 1024: ns.ROUTE_LINES, 56: ns.ROUTE_TWOLEVEL, 88: ns.ROUTE_TWOLEVEL, 104: ns.ROUTE_TWOLEVEL,
            1040: ns.ROUTE_TWOLEVEL, 2560: ns.ROUTE_TWOLEVEL, 2688: ns.ROUTE_TWOLEVEL, 4096: ns.ROUTE_TWOLEVEL, 136: ns.ROUTE_DENSE, 34: ns.ROUTE_DENSE,
            47: 0, 4098: 0, 0: 0}
    assert {L: ns.route(L) for L in want} == want
    monkeypatch.setenv("IMCOM_NOISEPS_ROUTE", "dense")
    assert ns.route(1040) == ns.ROUTE_DENSE and ns.route(48) == ns.ROUTE_DENSE and ns.route(47) == 0


def test_refusals(ns):
    from pyimcom_amd import _lib

    out = np.zeros(4, dtype=np.int64)
    for L, bin8 in ((47, 0), (52, 1), (4104, 1), (0, 0)):
        assert _lib.lib.imcom_noiseps_sizes(L, 1, bin8, 0, _lib.ptr(out)) == -1, (L, bin8)
    assert _lib.lib.imcom_noiseps_sizes(56, 1, 1, ns.ROUTE_LINES, _lib.ptr(out)) == -1  # 56 is no butterfly side
    assert _lib.lib.imcom_noiseps_sizes(56, 0, 1, 0, _lib.ptr(out)) == -1
    for shape, bin8 in (((47, 47), False), ((52, 52), True), ((4104, 4104), True), ((3, 48, 40), True)):
        with pytest.raises(ValueError):
            ns.power_spectrum_2d(np.zeros(shape, dtype=np.float32), bin8=bin8)
    with pytest.raises(ValueError):
        ns.power_spectrum_2d(np.zeros((48, 48), dtype=np.float32), window=np.ones((48, 40)))
    with pytest.raises(ValueError):
        ns.azimuthal_average(np.zeros((6, 6)), 3, ridx=np.arange(0, 3))
    with pytest.raises(ValueError):
        ns.azimuthal_average(np.zeros((6, 6)), 3, rbin=np.zeros((5, 5), dtype=int))


def test_byte_plan(ns, monkeypatch):
    monkeypatch.delenv("IMCOM_NOISEPS_ROUTE", raising=False)
    for L in (56, 1040, 2560):
        one, two = ns._sizes(L, 1, True), ns._sizes(L, 2, True)
        assert one[1] == L // 8 and ns._sizes(L, 1, False)[1] == L
        assert one[3] == (L // 2 + 1) * L * 16
        assert two[2] - one[2] >= 2 * one[3] - 512 and two[2] > one[2] >= 2 * one[3]  # H and F per frame (takes are aligned to 256 bytes)
        assert ns._sizes(L, 1, True, ns.ROUTE_DENSE)[2] > one[2] and ns._sizes(L, 1, True, ns.ROUTE_DENSE)[0] == ns.ROUTE_DENSE
    k = ns._plan_frames(2560, 6, True, 0, int(ns._sizes(2560, 3, True)[2] / ns.FILL) + 1)
    assert k == 3
    with pytest.raises(MemoryError):
        ns._plan_frames(2560, 6, True, 0, 1 << 20)
