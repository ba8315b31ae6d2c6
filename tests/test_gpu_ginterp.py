"""GPU parity of the pyimcom.meta.ginterp drop-in (pyimcom_amd/ginterp.py, csrc/ginterp.hip) against the reference's own outputs
(tests/golden/ginterp.npz, make_golden_ginterp.py), an analytic known answer, and the fused resampler against the matrix form at scale."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["a6", "a45"])
def test_interp_matrix_golden(golden, name):
    """(a) Rsearch 6 / samp 4.71 is the cond(Ad) ~ 1e11 case; Rsearch 4.5 has Cxy != 0 and stest 3.  The bounds sit above the spread
    of valid Cholesky solve orders (T 6e-7, U 1e-15, Sigma 4e-7)."""
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    Rs, samp, cxx, cxy, cyy, stest = g[f"{name}_pars"]
    posx, posy, T, U, S = ginterp.InterpMatrix(Rs, samp, g[f"{name}_x"], g[f"{name}_y"], [cxx, cxy, cyy], stest=int(stest))
    assert posx.dtype == np.int16 and np.array_equal(posx, g[f"{name}_posx"]) and np.array_equal(posy, g[f"{name}_posy"])
    assert T.shape == g[f"{name}_T"].shape and U.shape == g[f"{name}_U"].shape and S.shape == g[f"{name}_S"].shape
    assert np.abs(T - g[f"{name}_T"]).max() <= 1e-5
    assert np.abs(U - g[f"{name}_U"]).max() <= 1e-13
    assert np.abs(S - g[f"{name}_S"]).max() <= 1e-5


def _check_resample(g, pre, out, mask, umax, smax):
    assert mask.dtype == bool and np.array_equal(mask, g[f"{pre}_outmask"])
    ref = g[f"{pre}_out"]
    assert out.dtype == ref.dtype and out.shape == ref.shape
    assert np.abs(out.astype(np.float64) - ref).max() <= 1e-5
    assert np.all(out[..., mask] == 0)
    ru, rs = g[f"{pre}_UmaxSmax"]
    # U is a difference of O(1) terms that leaves ~1e-12: its absolute error is bounded as in the matrix form (1e-13), not relatively
    assert abs(umax - ru) <= max(1e-4 * abs(ru), 1e-13)
    assert abs(smax - rs) <= 1e-5


def test_multi_interp_golden_f32_layers(golden):
    """(b) float32 layers, scattered mask, rotated + sheared map off the edges, chunks of 1000 with stest 3."""
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    Rs, samp, cxx, cxy, cyy, stest, bs = g["b_pars"]
    out, mask, umax, smax = ginterp.MultiInterp(g["b_in"], g["b_mask"], tuple(g["b_size"]), g["b_origin"], g["b_transform"], Rs, samp, [cxx, cxy, cyy],
                                                stest=int(stest), blocksize=int(bs))
    assert out.ndim == 3 and out.dtype == np.float32
    _check_resample(g, "b", out, mask, umax, smax)


def test_multi_interp_chunk_rule_of_umax_smax(golden):
    """(e) Umax / Smax over the points whose index within their blocksize chunk is a multiple of stest: here that rule and the plain
    every-stest-th rule pick cells of different fractions, and the reference's Smax differs by 5e-3 between them (the tolerance 1e-5)."""
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    args = (np.zeros((40, 80), dtype=bool), (3, 60), np.array([10.5, 15.25]), np.array([[0.5, 0.0], [0.0, 1.0]]), 6.0, 4.71, [0.3, 0.0, 0.3])
    for bs, key in [(7, "e_UmaxSmax_chunks"), (10**7, "e_UmaxSmax_one_chunk")]:
        _, _, umax, smax = ginterp.MultiInterp(g["e_in"], *args, stest=2, blocksize=bs)
        ru, rs = g[key]
        assert abs(umax - ru) <= max(1e-4 * abs(ru), 1e-13) and abs(smax - rs) <= 1e-5, (bs, umax, smax, ru, rs)
    assert abs(g["e_UmaxSmax_chunks"][1] - g["e_UmaxSmax_one_chunk"][1]) > 1e-3


def test_multi_interp_maps_out_of_reach_are_masked(golden):
    """(f) A non-finite origin or Jacobian, or an origin beyond the int32 range: every pixel is masked and zero, Umax = Smax = 0, as
    the reference returns -- and nothing is read outside the input."""
    import torch

    from pyimcom_amd import ginterp

    g = golden("ginterp")
    msk = np.zeros((40, 40), dtype=bool)
    for mp, (ru, rs) in zip(g["f_maps"], g["f_UmaxSmax"]):
        out, mask, umax, smax = ginterp.MultiInterp(g["f_in"], msk, (8, 8), mp[:2], mp[2:].reshape(2, 2), 6.0, 4.71, [0.3, 0.0, 0.3])
        assert mask.all() and not out.any() and (umax, smax) == (ru, rs) == (0.0, 0.0), mp
    out, mask, umax, smax = ginterp.MultiInterp(torch.as_tensor(g["f_in"], device="cuda:0"), torch.zeros((40, 40), dtype=torch.bool, device="cuda:0"),
                                                (8, 8), [np.inf, 20.0], np.identity(2), 6.0, 4.71, [0.3, 0.0, 0.3])
    assert bool(mask.all()) and not bool(out.any()) and umax == 0.0 and smax == 0.0


def test_multi_interp_golden_2d_f64_identity(golden):
    """(c) a 2-D float64 input, identity map, integer origin: every fraction is exactly 0."""
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    Rs, samp, cxx, cxy, cyy = g["c_pars"]
    out, mask, umax, smax = ginterp.MultiInterp(g["c_in"], g["c_mask"], tuple(g["c_size"]), g["c_origin"], np.identity(2), Rs, samp, [cxx, cxy, cyy])
    assert out.ndim == 2 and out.dtype == np.float64
    _check_resample(g, "c", out, mask, umax, smax)


def test_multi_interp_early_exit(golden):
    """(d) 2 bb >= min(nx_in, ny_in): all zeros, everything masked, Umax = Smax = 0, exactly."""
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    out, mask, umax, smax = ginterp.MultiInterp(g["d_in"], g["d_mask"], (5, 7), np.array([2.0, 2.0]), np.identity(2), 6.0, 4.71, [0.3, 0.0, 0.3])
    assert out.dtype == np.float32 and np.array_equal(out, g["d_out"]) and np.array_equal(mask, g["d_outmask"])
    assert umax == 0.0 and smax == 0.0


def test_unsupported_radius_is_refused():
    """Beyond the built range: IMCOM_ERR_UNSUPPORTED (-4), decided before any geometry is built for a far-off radius; NaN: IMCOM_ERR_ARG."""
    from pyimcom_amd import _lib, ginterp

    for Rs, status in [(12.0, -4), (1.0e5, -4), (float("nan"), -1), (-1.0, -1)]:
        with pytest.raises(_lib.ImcomError) as e:
            ginterp.InterpMatrix(Rs, 4.71, np.array([0.5]), np.array([0.5]), [0.3, 0.0, 0.3])
        assert e.value.status == status, Rs
        with pytest.raises(_lib.ImcomError) as e:
            ginterp.MultiInterp(np.ones((40, 40), dtype=np.float32), np.zeros((40, 40), dtype=bool), (4, 4), [20.0, 20.0], np.identity(2), Rs, 4.71,
                                [0.3, 0.0, 0.3])
        assert e.value.status == status, Rs


def test_known_answer_cosines_and_ring():
    """The reference's analytic test (tests/pyimcom/test_meta.py), in our own words: cosine layers are mapped and damped by the extra
    smoothing, a ring of unit Gaussians becomes Gaussians of width sigma / sc scaled by 1 / det(M / sc)."""
    from pyimcom_amd import ginterp

    samp, Rs, n, nout, sc = 5.0, 4.5, 425, 720, 0.5
    sigma = samp / np.sqrt(8.0 * np.log(2.0))
    u0, v0 = 0.243, 0.128
    M = np.array([[0.52, 0.005], [-0.015, 0.51]])
    origin = np.array([6.0, 3.0])
    eC = (M @ M.T / sc**2 - np.identity(2)) * sigma**2
    C = [eC[0, 0], eC[0, 1], eC[1, 1]]
    yy, xx = np.mgrid[:n, :n].astype(np.float64)
    ring = [(200 + 150 * np.cos(k * np.pi / 32), 170 + 150 * np.sin(k * np.pi / 32)) for k in range(64)]
    img = np.zeros((6, n, n), dtype=np.float32)
    for j in range(4):
        img[j] = 1.0 + 0.1 * np.cos(2 * np.pi * (u0 * xx + v0 * yy) / 2.0**j)
    img[4] = img[:4].sum(axis=0) - 3.6
    for xc, yc in ring:
        img[5] += np.exp(-0.5 * ((xx - xc) ** 2 + (yy - yc) ** 2) / sigma**2)
    out, mask, _, _ = ginterp.MultiInterp(img, np.zeros((n, n), dtype=bool), (nout, nout), origin, M, Rs, samp, C)

    yo, xo = np.mgrid[:nout, :nout].astype(np.float64)
    xin = M[0, 0] * xo + M[0, 1] * yo + origin[0]
    yin = M[1, 0] * xo + M[1, 1] * yo + origin[1]
    damp = np.exp(-2 * np.pi**2 * (u0**2 * C[0] + 2 * u0 * v0 * C[1] + v0**2 * C[2]))
    want = np.zeros((6, nout, nout))
    for j in range(4):
        want[j] = 1.0 + 0.1 * np.cos(2 * np.pi * (u0 * xin + v0 * yin) / 2.0**j) * damp ** (0.25**j)
    want[4] = want[:4].sum(axis=0) - 3.6
    Minv, scale = np.linalg.inv(M), 1.0 / np.linalg.det(M / sc)
    for xc, yc in ring:
        xt, yt = Minv @ (np.array([xc, yc]) - origin)
        want[5] += scale * np.exp(-0.5 * ((xo - xt) ** 2 + (yo - yt) ** 2) / (sigma / sc) ** 2)
    diff = np.where(mask, 0.0, out - want)
    assert (~mask).sum() > 0.5 * mask.size
    assert np.abs(diff).max() < 4e-5
    assert np.abs(diff[1]).max() < 1e-5 and np.abs(diff[5]).max() < 1e-5


def test_fused_resampler_matches_matrix_form_at_scale():
    """Rsearch 6, 2048^2 outputs, 8 float32 layers: the fused resampler against the matrix form of the same points plus a float64 host
    gather on 2000 random output pixels; a torch call on the device gives the same bits as the numpy call."""
    import torch

    from pyimcom_amd import ginterp

    rng = np.random.default_rng(7)
    n_in, nout, nl, Rs, samp, C = 1100, 2048, 8, 6.0, 4.71, [0.25, 0.01, 0.2]
    img = (1.0 + 0.2 * rng.standard_normal((nl, n_in, n_in))).astype(np.float32)
    msk = rng.random((n_in, n_in)) < 1e-4
    th = 0.4
    M = 0.5 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1.0, 0.03], [0.0, 1.02]])
    origin = np.array([420.25, 3.5])
    out, mask, umax, smax = ginterp.MultiInterp(img, msk, (nout, nout), origin, M, Rs, samp, C)
    assert out.shape == (nl, nout, nout) and 0.2 * mask.size < (~mask).sum()

    pix = rng.choice(nout * nout, 2000, replace=False)
    yo, xo = (pix // nout).astype(np.float64), (pix % nout).astype(np.float64)
    xin = M[0][0] * xo + M[0][1] * yo + origin[0]
    yin = M[1][0] * xo + M[1][1] * yo + origin[1]
    xi, yi = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    posx, posy, T, U, S = ginterp.InterpMatrix(Rs, samp, xin - xi, yin - yi, C)
    ok = ~mask.ravel()[pix]
    xi, yi, T = xi[ok], yi[ok], T[ok]
    ref = np.einsum("pk,lpk->lp", T, img[:, yi[:, None] + posy[None, :], xi[:, None] + posx[None, :]].astype(np.float64))
    got = out.reshape(nl, -1)[:, pix[ok]]
    assert ok.sum() > 500 and np.abs(got - ref).max() <= 1e-5
    assert 0.0 < umax and U.max() <= umax * (1 + 1e-6) and S.max() <= smax + 1e-12

    tout, tmask, tumax, tsmax = ginterp.MultiInterp(torch.as_tensor(img, device="cuda:0"), torch.as_tensor(msk, device="cuda:0"), (nout, nout), origin, M,
                                                    Rs, samp, C)
    assert isinstance(tout, torch.Tensor) and tout.device.type == "cuda" and tout.dtype == torch.float32
    assert np.array_equal(tout.cpu().numpy(), out) and np.array_equal(tmask.cpu().numpy(), mask)
    assert tumax == umax and tsmax == smax
