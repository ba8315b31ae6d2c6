"""numpy / scipy restatement of the arithmetic of run_imsubtract_single (reference src/pyimcom/splitpsf/imsubtract.py:689-707) for shapes
too big for a committed fixture.  tests/test_imsubtract_host.py pins it to tests/golden/imsubtract.npz, which the reference's own code
produced.  Test-side only: nothing under pyimcom_amd/ imports it."""

import numpy as np
from scipy.signal import fftconvolve
from scipy.special import eval_legendre


def geometry(axis_num, oversamp, nside):
    """imsubtract.py:387-389, 451."""
    I_pad = int(np.ceil(axis_num / 2 / oversamp))
    return I_pad, (oversamp + 2 * oversamp * I_pad - axis_num) // 2, oversamp * (nside + 2 * I_pad)


def u_canvas(axis_num, oversamp, nside):
    """imsubtract.py:487-488."""
    I_pad, _, A = geometry(axis_num, oversamp, nside)
    x = np.linspace(-I_pad - 0.5 + 0.5 / oversamp, nside + I_pad - 0.5 - 0.5 / oversamp, A)
    return (x - (nside - 1) / 2) / (nside / 2)


def modulated(canvas, u, lu, lv):
    """imsubtract.py:694-696: float32 products, the x factor first."""
    arr = np.copy(canvas)
    arr *= eval_legendre(lu, u).astype(np.float32)[None, :]
    arr *= eval_legendre(lv, u).astype(np.float32)[:, None]
    return arr


def kh_full(canvas, K, oversamp, nside, Nl, dtype=np.float64):
    """The reference's loop as it stands (full resolution, then decimated): float64 transforms per term, accumulated in ``dtype``
    (float32 is what the reference's KH is)."""
    ax = K.shape[1]
    _, first, A = geometry(ax, oversamp, nside)
    u = u_canvas(ax, oversamp, nside)
    KH = np.zeros((A - ax + 1, A - ax + 1), dtype=dtype)
    for lu in range(Nl):
        for lv in range(Nl):
            KH += fftconvolve(K[lu + lv * Nl].astype(np.float64), modulated(canvas, u, lu, lv).astype(np.float64), mode="valid")
    return KH[first:-first:oversamp, first:-first:oversamp]


def kh_phases(canvas, K, oversamp, nside, Nl):
    """The same samples without the full-resolution array: oversamp^2 phases per term, each a small float64 convolution of a sub-image of
    the canvas.  Kernel rows j = oversamp j' + p meet the canvas rows congruent to first_index + ax - 1 - p."""
    s, ax = oversamp, K.shape[1]
    _, first, A = geometry(ax, s, nside)
    u = u_canvas(ax, s, nside)
    npk = ax // s
    out = np.zeros((nside, nside))
    for lu in range(Nl):
        for lv in range(Nl):
            arr = modulated(canvas, u, lu, lv).astype(np.float64)
            Kc = K[lu + lv * Nl].astype(np.float64)
            for p in range(s):
                ep = first + ax - 1 - p
                for q in range(s):
                    eq = first + ax - 1 - q
                    sub = arr[ep % s::s, eq % s::s]
                    by, bx = ep // s - (npk - 1), eq // s - (npk - 1)
                    sub = sub[by:by + nside + npk - 1, bx:bx + nside + npk - 1]
                    out += fftconvolve(sub, Kc[p::s, q::s], mode="valid")
    return out


def kh_brute(canvas, K, oversamp, nside, Nl, samples):
    """The defining sum (float64) at a few samples [(Y, X), ...]: the check of everything above."""
    s, ax = oversamp, K.shape[1]
    _, first, A = geometry(ax, s, nside)
    u = u_canvas(ax, s, nside)
    out = np.zeros(len(samples))
    for lu in range(Nl):
        for lv in range(Nl):
            arr = modulated(canvas, u, lu, lv).astype(np.float64)
            Kc = K[lu + lv * Nl].astype(np.float64)[::-1, ::-1]
            for k, (Y, X) in enumerate(samples):
                y, x = first + s * Y, first + s * X
                out[k] += np.sum(Kc * arr[y:y + ax, x:x + ax])
    return out


def subtract(image, kh):
    """imsubtract.py:707 with the sums rounded once."""
    return (image.astype(np.float64) - kh).astype(np.float32)
