"""CPU-side checks of the injected star-grid layer (pyimcom_amd/inject.py): the numpy restatement the device is compared with at full
size (tests/inject_reference.py) pinned to the reference's own outputs (tests/golden/inject.npz, make_golden_inject.py), the Legendre
coefficients, the chip test, the chunk planner and the argument checks that need no device.

The bound of every image comparison is the one the composition of the two stages gives: smooth_and_pad is asserted within 2e-14 * max
(test_smooth_and_pad_golden) and one axis of the D5512 taps amplifies an input error by at most max_fh sum_k |w_k(fh)| = 1.5785 (at
fh = 0; computed from the coefficients by test_weight_gain below), 2.4917 for the two axes, so 2.5 * 2e-14 = 5e-14 of
oversamp^2 max|PSF| per star and, two overlapping boxes on a pixel, 1e-13 * max|image|."""

import ctypes as C

import numpy as np
import pytest

from tests import inject_reference as ref

IMAGE_RTOL = 1.0e-13
PSF_RTOL = 2.0e-14
CONFIGS = ("anlsim", "l2")


def test_weight_gain():
    g = ref.weight_gain()
    assert 1.57 < g < 1.58 and g * g <= 2.5
    assert abs(np.abs(ref.getw(np.array(0.0))).sum() - g) < 1e-12  # largest at fh = 0


def test_restatement_weights_match_reference(golden):
    g = golden("getw")
    fh = g["fh"]
    assert np.max(np.abs(ref.getw(fh) - g["w"])) <= 4 * np.finfo(np.float64).eps


@pytest.mark.parametrize("name", CONFIGS)
def test_restatement_psfs_match_golden(golden, name):
    g = golden("inject")
    tw, scale = g[f"{name}_pars"]
    want = g[f"{name}_psfs"]
    got = ref.psf_from_cube(g["cube"], g["lpoly"], tw, 0.0, scale)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"{name}: restatement PSFs vs golden {err:.3e}")
    assert got.shape == want.shape and err <= PSF_RTOL


@pytest.mark.parametrize("name", CONFIGS)
def test_restatement_image_matches_golden(golden, name):
    """From the golden PSFs (the drawing alone) and from the cube (both stages)."""
    g = golden("inject")
    tw, scale = g[f"{name}_pars"]
    want = g[f"{name}_image"]
    nside, os_ = int(g["nside"]), int(g["oversamp"])
    a = ref.draw_stars(g[f"{name}_psfs"], g["xsca"], g["ysca"], nside, os_)
    b = ref.star_image(g["cube"], g["lpoly"], g["xsca"], g["ysca"], nside, os_, tw, scale)
    ea, eb = (np.max(np.abs(x - want)) / np.max(np.abs(want)) for x in (a, b))
    print(f"{name}: restatement image vs golden: drawing {ea:.3e}, cube + drawing {eb:.3e}")
    assert ea <= IMAGE_RTOL and eb <= IMAGE_RTOL
    assert np.array_equal(a != 0, want != 0)  # the same pixels are touched


def test_fixture_covers_the_cases(golden):
    g = golden("inject")
    x, y, nside = g["xsca"], g["ysca"], int(g["nside"])
    keep = ref.on_chip(x, y, nside)
    assert (~keep).sum() == 2 and keep.sum() == 11
    assert (x < 0).any() and (y < 0).any() and (x > nside).any() and (y > nside).any()
    assert ((x == np.round(x)) & (y == np.round(y)) & keep).any()
    img = g["anlsim_image"]
    assert img[:, 0].any() and img[0].any() and img[:, -1].any() and img[-1].any()  # clipped at all four edges


def _lpoly_tol(po, u, v):
    """InImage.LPolyArr evaluates scipy's legendre(m) polynomials by Horner's rule from coefficients that carry a few ulps themselves;
    the recurrence of lpoly_arr differs from that in rounding only.  For order m <= 4 the coefficients sum to at most (35 + 30 + 3) / 8 =
    8.5 in magnitude, Horner's rule and the coefficient errors come to about 3 m <= 12 roundings, and there are two factors: 24 * 8.5 eps
    on -1 .. +1, growing as |x|^m per factor outside it."""
    grow = np.maximum(1.0, np.abs(u)) ** po * np.maximum(1.0, np.abs(v)) ** po
    return 24 * 8.5 * np.finfo(np.float64).eps * grow[:, None]


def test_lpoly_arr_matches_reference(golden):
    from pyimcom_amd import inject

    g = golden("inject")
    assert np.all(np.abs(inject.lpoly_arr(2, g["u"], g["v"]) - g["lpoly"]) <= _lpoly_tol(2, g["u"], g["v"]))
    for po in (0, 1, 3, 4):
        u, v = g["lp_pts"][:, 0], g["lp_pts"][:, 1]
        got = inject.lpoly_arr(po, u, v)
        assert got.shape == (7, (po + 1) ** 2)
        assert np.all(np.abs(got - g[f"lp_{po}"]) <= _lpoly_tol(po, u, v))
    assert np.array_equal(inject.lpoly_arr(2, g["u"], g["v"]), ref.lpoly_arr(2, g["u"], g["v"]))


def test_on_chip_follows_int_truncation():
    from pyimcom_amd import inject

    x = np.array([-63.5, -64.5, -0.5, 4151.9, 4152.0, 100.0, np.nan, np.inf, 100.0])
    y = np.array([100.0, 100.0, -63.9, 100.0, 100.0, 4152.5, 100.0, 100.0, -64.0])
    # int(-63.5) = -63 -> box [-127, 1): one column; int(-64.5) = -64 -> [-128, 0): none; int(4151.9) - 64 = 4087 < 4088
    want = [True, False, True, True, False, False, False, False, False]
    assert inject.on_chip(x, y, 4088).tolist() == want
    assert ref.on_chip(x[:6], y[:6], 4088).tolist() == want[:6]
    for xs, ys, w in zip(x[:6], y[:6], want):  # the reference's own arithmetic (layer.py:827-834)
        pnx = min(4088, int(xs) + 64) - max(0, int(xs) - 64)
        pny = min(4088, int(ys) + 64) - max(0, int(ys) - 64)
        assert (pnx >= 1 and pny >= 1) == w


def test_plan_chunk_counts_bytes():
    from pyimcom_amd import inject

    per = 8 * (80 * 80 + 2 + 16)
    fixed = inject._cube_workspace_bytes(16, 64, 64, 8)
    assert inject.plan_chunk(1200, (80, 80), 16, (64, 64), 8, free_bytes=10**10) == 1200
    n = inject.plan_chunk(1200, (80, 80), 16, (64, 64), 8, free_bytes=int((fixed + 100.5 * per) / inject.FILL))
    assert n == 100
    with pytest.raises(MemoryError):
        inject.plan_chunk(1200, (80, 80), 16, (64, 64), 8, free_bytes=1000)


def test_signature_matches_reference():
    import inspect

    from pyimcom_amd import inject

    p = list(inspect.signature(inject.make_image_from_grid).parameters)
    assert p[:7] == ["res", "inpsf", "idsca", "obsdata", "mywcs", "nside_sca", "inpsf_oversamp"] and p[7:] == ["star_grid"]


@pytest.mark.parametrize("name", ["imcom_psf_from_cube", "imcom_draw_stars"])
def test_null_context_is_refused(name):
    from pyimcom_amd import _lib

    args = [0.0 if t is C.c_double else 0 if t in (C.c_int, C.c_long) else None for t in _lib.SIGNATURES[name]]
    assert getattr(_lib.lib, name)(*args) == -1  # IMCOM_ERR_ARG
    assert "null context" in _lib.lib.imcom_last_error().decode()


def test_python_argument_checks():
    from pyimcom_amd import inject

    with pytest.raises(ValueError):
        inject.star_image([1.0], [1.0], 64, 4)  # no PSF source
    with pytest.raises(ValueError):
        inject.star_image([1.0], [1.0], 64, 4, psf=np.zeros((8, 8)), psf_fn=lambda i: None)
    with pytest.raises(ValueError):
        inject.lpoly_arr(2, np.zeros(3), np.zeros(4))
