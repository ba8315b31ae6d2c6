"""pyimcom_amd.inject on the device: imcom_psf_from_cube and imcom_draw_stars (csrc/inject.hip) against the reference's own outputs
(tests/golden/inject.npz) and, at full size, against the numpy restatement that tests/test_inject_host.py pins to the same golden.

Bounds (set by the composition of the two stages, not by what the device gives; see tests/test_inject_host.py): an image within
1e-13 * max|reference image|: smooth_and_pad's asserted 2e-14, times the D5512 taps' gain (sum |w|)^2 = 1.5785^2 = 2.4917 <= 2.5
(largest at fh = 0, computed from the coefficients on the CPU by test_weight_gain), times two for overlapping boxes.  A PSF formed from
smeared planes within 2e-14 * scale * sum_a |lpoly_a| max|cube_a|: every plane carries smooth_and_pad's bound on its own scale."""

import types

import numpy as np
import pytest

from tests import inject_reference as ref

pytestmark = pytest.mark.gpu

IMAGE_RTOL = 1.0e-13
SMOOTH_RTOL = 2.0e-14
CONFIGS = ("anlsim", "l2")


def _psf_tol(cube, lpoly, scale):
    return SMOOTH_RTOL * abs(scale) * (np.abs(lpoly) @ np.abs(cube).max(axis=(1, 2)))[:, None, None]


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("name", CONFIGS)
def test_psf_from_cube_golden(golden, name):
    import torch

    from pyimcom_amd import inject

    g = golden("inject")
    tw, scale = g[f"{name}_pars"]
    want, tol = g[f"{name}_psfs"], _psf_tol(g["cube"], g["lpoly"], scale)
    host = inject.psf_from_cube(g["cube"], g["lpoly"], tw, 0.0, scale)
    dev = inject.psf_from_cube(torch.as_tensor(g["cube"], device="cuda:0"), torch.as_tensor(g["lpoly"], device="cuda:0"), tw, 0.0, scale)
    assert isinstance(host, np.ndarray) and dev.is_cuda and host.shape == want.shape
    print(f"{name}: psf_from_cube vs golden {_rel(host, want):.3e} of max (bound {float(tol.max() / np.abs(want).max()):.3e})")
    assert np.all(np.abs(host - want) <= tol)
    assert np.array_equal(dev.cpu().numpy(), host)


@pytest.mark.parametrize("name", CONFIGS)
def test_draw_stars_golden(golden, name):
    import torch

    from pyimcom_amd import inject

    g = golden("inject")
    want = g[f"{name}_image"]
    nside, os_ = int(g["nside"]), int(g["oversamp"])
    keep = ref.on_chip(g["xsca"], g["ysca"], nside)
    for sel in (slice(None), keep):  # stars off the chip draw nothing, whether the caller drops them or not
        psfs, x, y = g[f"{name}_psfs"][sel], g["xsca"][sel], g["ysca"][sel]
        host = inject.draw_stars(psfs, x, y, nside, os_)
        dev = inject.draw_stars(torch.as_tensor(psfs, device="cuda:0"), torch.as_tensor(x, device="cuda:0"), y, nside, os_)
        print(f"{name}: draw_stars vs golden {_rel(host, want):.3e}")
        assert _rel(host, want) <= IMAGE_RTOL
        assert np.array_equal(dev.cpu().numpy(), host)
        assert np.array_equal(host != 0, want != 0)
    base = np.full((nside, nside), 0.25)  # the stars are ADDED to what the image holds
    got = inject.draw_stars(g[f"{name}_psfs"], g["xsca"], g["ysca"], nside, os_, out=base.copy())
    assert np.max(np.abs(got - (want + 0.25))) <= IMAGE_RTOL * np.max(np.abs(want)) + 2 * np.finfo(np.float64).eps


class _Wcs:
    """all_world2pix of the duck-typed InImage: "ra" is the star's index; the pixel it returns scales back to the fixture's u, v."""

    def __init__(self, u, v):
        self.u, self.v = u, v

    def all_world2pix(self, ra, dec, origin):
        i = np.asarray(ra).astype(int)
        return self.u[i] * 2044.0 + 2043.5, self.v[i] * 2044.0 + 2043.5


class _InImage:
    def __init__(self, g, name, fmt, fixed=None):
        self.g, self.name, self.fixed, self.calls = g, name, fixed, []
        self.blk = types.SimpleNamespace(cfg=types.SimpleNamespace(inpsf_format=fmt, inpsfdraw_format=None, inpsf_oversamp=int(g["oversamp"]),
                                                                    psfsplit=False))
        self.inwcs = _Wcs(g["u"], g["v"])

    def get_psf_pos(self, pos, use_shortrange=False, use_drawpsf=False):
        assert use_drawpsf
        i = int(round(pos[0]))
        self.calls.append(i)
        if self.blk.cfg.inpsf_format in ("anlsim", "L2_2506"):
            self.inpsf_cube = self.g["cube"]
        return self.g[f"{self.name}_psfs"][i if self.fixed is None else self.fixed]


def _grid(g):
    n = g["xsca"].size
    return lambda res, wcs: (np.arange(n), g["xsca"], g["ysca"], np.arange(n, dtype=np.float64), np.zeros(n))


def test_make_image_from_grid_three_sources(golden):
    from pyimcom_amd import inject

    g = golden("inject")
    nside, os_ = int(g["nside"]), int(g["oversamp"])
    want = g["anlsim_image"]
    on = set(np.nonzero(ref.on_chip(g["xsca"], g["ysca"], nside))[0].tolist())
    # 1. the Legendre cube, formed on the device: one call to get_psf_pos (it loads the cube), none per star
    im = _InImage(g, "anlsim", "anlsim")
    got = inject.make_image_from_grid(14, im.get_psf_pos, (0, 1), None, None, nside, os_, star_grid=_grid(g))
    print(f"cube source vs golden {_rel(got, want):.3e}")
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (nside, nside)
    assert _rel(got, want) <= IMAGE_RTOL and len(im.calls) == 1
    # 2. a callable per star (piff): a plain function, called for the stars that reach the chip and no others
    calls = []

    def inpsf(pos, use_drawpsf=False):
        calls.append(int(round(pos[0])))
        return g["anlsim_psfs"][calls[-1]]

    got = inject.make_image_from_grid(14, inpsf, (0, 1), None, None, nside, os_, star_grid=_grid(g))
    print(f"callable source vs golden {_rel(got, want):.3e}")
    assert _rel(got, want) <= IMAGE_RTOL and set(calls) == on
    # 3. one PSF for all stars (dc2_imsim): the restatement (pinned to the golden by test_inject_host) with that PSF
    im = _InImage(g, "anlsim", "dc2_imsim", fixed=0)
    got = inject.make_image_from_grid(14, im.get_psf_pos, (0, 1), None, None, nside, os_, star_grid=_grid(g))
    fixed = ref.draw_stars(g["anlsim_psfs"][0], g["xsca"], g["ysca"], nside, os_)
    print(f"fixed source vs restatement {_rel(got, fixed):.3e}")
    assert _rel(got, fixed) <= IMAGE_RTOL and len(im.calls) == 1
    # star_image with the other format's parameters (top-hat width 0, no scale)
    tw, scale = g["l2_pars"]
    got = inject.star_image(g["xsca"], g["ysca"], nside, os_, cube=g["cube"], lpoly=g["lpoly"], tophatwidth=tw, scale=scale).cpu().numpy()
    assert _rel(got, g["l2_image"]) <= IMAGE_RTOL


def _lattice(nside, spacing, rng):
    """A jittered lattice of `spacing` pixels reaching one chip side beyond the chip on every side."""
    t = np.arange(-nside, 2 * nside, spacing, dtype=np.float64)
    xx, yy = np.meshgrid(t, t)
    return (xx + rng.uniform(-20, 20, xx.shape)).ravel(), (yy + rng.uniform(-20, 20, yy.shape)).ravel()


def _cube(na, n, rng):
    yy, xx = np.mgrid[:n, :n] - (n - 1) / 2.0
    cube = np.zeros((na, n, n))
    cube[0] = np.exp(-(xx**2 + yy**2) / (2 * 7.0**2))
    cube[0] *= 64.0 / cube[0].sum()
    for a in range(1, na):
        cube[a] = 0.05 * cube[0] * rng.standard_normal((n, n)) / (1 + a)
    return cube


def test_full_size_against_restatement(monkeypatch):
    """One SCA: 4088^2, a 16-plane cube, oversamp 8, a lattice of 117 px spacing (HEALPix resolution 14) over 3 x 3 chip areas."""
    from pyimcom_amd import inject

    rng = np.random.default_rng(5)
    nside, os_, d = 4088, 8, 64
    x, y = _lattice(nside, 117.0, rng)
    cube = _cube(16, 64, rng)
    lpoly = inject.lpoly_arr(3, (x - 2043.5) / 2044.0, (y - 2043.5) / 2044.0)
    # the reference's own test, star by star (layer.py:827-834)
    drawn = np.array([min(nside, int(a) + d) - max(0, int(a) - d) >= 1 and min(nside, int(b) + d) - max(0, int(b) - d) >= 1 for a, b in zip(x, y)])
    formed = []
    real = inject.psf_from_cube
    monkeypatch.setattr(inject, "psf_from_cube", lambda cube_, lp, *a, **k: (formed.append(int(lp.shape[0])), real(cube_, lp, *a, **k))[1])
    got = inject.star_image(x, y, nside, os_, cube=cube, lpoly=lpoly, scale=1.0 / 64.0).cpu().numpy()
    skipped = 1.0 - sum(formed) / x.size
    print(f"{x.size} stars, {int(drawn.sum())} reach the chip, PSFs formed {sum(formed)}, skipped share {skipped:.4f}")
    assert sum(formed) == int(drawn.sum())  # no star on the chip is skipped, no PSF is formed for one off it
    assert abs(skipped - (1.0 - drawn.mean())) < 1e-12 and 0.8 < skipped < 0.9  # (4088 + 128)^2 / 12264^2 of the area is kept
    want = ref.star_image(cube, lpoly, x, y, nside, os_, float(os_), 1.0 / 64.0, d)
    print(f"full size vs restatement {_rel(got, want):.3e}")
    assert _rel(got, want) <= IMAGE_RTOL
    assert np.array_equal(got != 0, want != 0)


def test_bit_identity():
    import torch

    from pyimcom_amd import inject

    rng = np.random.default_rng(9)
    nside, os_ = 600, 4
    x, y = _lattice(nside, 47.0, rng)  # boxes of neighbours overlap several times over; the PSF patches overlap too
    on = np.nonzero(inject.on_chip(x, y, nside))[0]
    x[on[3]], y[on[3]] = x[on[50]], y[on[50]]  # and two stars on one spot
    cube = _cube(9, 40, rng)
    lpoly = inject.lpoly_arr(2, (x - 300.0) / 300.0, (y - 300.0) / 300.0)
    kw = dict(cube=cube, lpoly=lpoly, scale=1.0)
    a = inject.star_image(x, y, nside, os_, **kw)
    assert torch.equal(a, inject.star_image(x, y, nside, os_, **kw))
    n_on = int(inject.on_chip(x, y, nside).sum())
    assert n_on > 150
    for chunk in (1, 64, n_on):
        assert torch.equal(a, inject.star_image(x, y, nside, os_, chunk=chunk, **kw)), chunk
    keep = inject.on_chip(x, y, nside)
    xs, ys = torch.as_tensor(x[keep], device="cuda:0"), torch.as_tensor(y[keep], device="cuda:0")
    psfs = inject.psf_from_cube(torch.as_tensor(cube, device="cuda:0"), torch.as_tensor(lpoly[keep], device="cuda:0"), float(os_), 0.0, 1.0)
    one = inject.draw_stars(psfs, xs, ys, nside, os_)
    assert torch.equal(one, a)
    for step in (1, 7, 100):
        out = torch.zeros_like(one)
        for s0 in range(0, n_on, step):
            inject.draw_stars(psfs[s0:s0 + step], xs[s0:s0 + step], ys[s0:s0 + step], nside, os_, out=out)
        assert torch.equal(out, one), step
    host = inject.draw_stars(psfs.cpu().numpy(), x[keep], y[keep], nside, os_)
    assert np.array_equal(host, one.cpu().numpy())


def test_small_box_clips_the_patch():
    """d below the PSF's reach: the box of layer.py:827-830 cuts the patch (the reference's d = 64 never does)."""
    from pyimcom_amd import inject

    rng = np.random.default_rng(2)
    cube = _cube(4, 40, rng)
    x, y = np.array([20.3, 41.0, -1.5, 63.2]), np.array([20.9, 40.0, 30.2, 62.1])
    psfs = ref.psf_from_cube(cube, inject.lpoly_arr(1, x / 64.0, y / 64.0), 4.0)
    for d in (1, 3, 64):
        got = inject.draw_stars(psfs, x, y, 64, 4, d=d)
        want = ref.draw_stars(psfs, x, y, 64, 4, d=d)
        assert _rel(got, want) <= IMAGE_RTOL and np.array_equal(got != 0, want != 0), d


@pytest.mark.parametrize("name", CONFIGS)
def test_smoothing_once_is_the_literal_form_in_rounding(golden, name):
    """Planes smeared once and contracted per star against the literal coadd.py:631 -- contract, then smear every star."""
    from pyimcom_amd import inject, psfs

    g = golden("inject")
    tw, scale = g[f"{name}_pars"]
    literal = scale * psfs.smooth_and_pad(np.einsum("sa,aij->sij", g["lpoly"], g["cube"]), tw, 0.0)
    got = inject.psf_from_cube(g["cube"], g["lpoly"], tw, 0.0, scale)
    tol = _psf_tol(g["cube"], g["lpoly"], scale) + SMOOTH_RTOL * np.abs(literal).max(axis=(1, 2))[:, None, None]  # each side carries its bound
    print(f"{name}: smeared planes vs literal {_rel(got, literal):.3e}")
    assert np.all(np.abs(got - literal) <= tol)


def test_arguments_are_checked():
    from pyimcom_amd import _lib, inject

    z = np.zeros((2, 8, 8))
    with pytest.raises(_lib.ImcomError):
        inject.draw_stars(z, np.zeros(2), np.zeros(2), 32, 0.0)
    with pytest.raises(_lib.ImcomError):
        inject.draw_stars(z, np.zeros(2), np.zeros(2), 32, float("nan"))
    with pytest.raises(_lib.ImcomError):
        inject.psf_from_cube(np.zeros((4, 8, 8)), np.zeros((2, 4)), -1.0)
    with pytest.raises(ValueError):
        inject.psf_from_cube(np.zeros((4, 8, 8)), np.zeros((2, 3)), 1.0)
    with pytest.raises(ValueError):
        inject.draw_stars(z, np.zeros(3), np.zeros(2), 32, 4)
    img = inject.draw_stars(z, np.array([np.nan, 1e300]), np.array([4.0, np.inf]), 32, 4)  # positions that are nowhere draw nothing
    assert not img.any()
