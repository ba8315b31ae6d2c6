"""Test infrastructure: the arithmetic of the reference's ``SplitPSF`` (src/pyimcom/splitpsf/splitpsf.py:71-284) restated with numpy and scipy,
pinned to the fixture tests/golden/splitpsf.npz (tests/test_splitpsf_host.py), plus the same with its transforms in extended precision
(``extended=True``: scipy.fft on numpy.longdouble) -- the yardstick of the reference's own rounding -- and a duck-typed WCS with shear and a
quadratic term.  Not part of the package: pyimcom_amd imports nothing from here."""

import numpy as np
import scipy.fft
import scipy.signal
from scipy.special import eval_legendre, roots_legendre


class ShearWCS:
    """A WCS stand-in with ``all_pix2world(xy, 0)``: a sheared, slightly non-linear map around (ra0, dec0), pixel scale about 0.11 arcsec."""

    def __init__(self, ra0=53.0, dec0=-40.0, nside=4088, shear=(0.04, -0.03), rot=0.3, quad=2.0e-6, scale=0.11 / 3600):
        self.ra0, self.dec0, self.nside, self.shear, self.rot, self.quad, self.scale = ra0, dec0, nside, shear, rot, quad, scale

    def all_pix2world(self, xy, origin):
        xy = np.asarray(xy, dtype=np.float64)
        x, y = xy[:, 0] - self.nside / 2.0, xy[:, 1] - self.nside / 2.0
        g1, g2 = self.shear
        c, s = np.cos(self.rot), np.sin(self.rot)
        u = (1 + g1) * x + g2 * y + self.quad * x * x
        v = g2 * x + (1 - g1) * y + self.quad * x * y
        xi, eta = self.scale * (c * u - s * v), self.scale * (s * u + c * v)
        dec = self.dec0 + eta
        ra = self.ra0 - xi / np.cos(np.radians(self.dec0))
        return np.stack([ra, dec], axis=1)


def window_blackman(x):
    alpha = 0.08
    return np.where(x >= 1, 1.0, np.where(x <= -1, 0.0, 0.5 * (x + 1) + (0.5 * np.sin(np.pi * x) + alpha / 4 * np.sin(2 * np.pi * x)) / ((1 - alpha) * np.pi)))


def window_2d(n, r1, r2):
    X_ = np.linspace((1 - n) / 2.0, (n - 1) / 2.0, n)
    xx, yy = np.meshgrid(X_, X_)
    return window_blackman(-1.0 + 2.0 / (r2 - r1) * (r2 - np.sqrt(xx**2 + yy**2)))


def truncate_2d(n, m):
    if m == 0:
        return np.ones((n, n))
    X_ = np.ones((n,))
    X_[:m] = window_blackman(np.linspace(-1.0, 1.0, m + 2))[1:-1]
    X_[-m:] = X_[m - 1::-1]
    return np.outer(X_, X_)


def _fft2(a, extended):
    return scipy.fft.fft2(a.astype(np.clongdouble)) if extended else np.fft.fft2(a)


def _ifft2(a, extended):
    return scipy.fft.ifft2(a.astype(np.clongdouble)) if extended else np.fft.ifft2(a)


def tophatfilter(cube, width, extended=False):
    npad = int(np.ceil(width))
    npad += (4 - npad) % 4
    nplane, ny, nx = cube.shape
    nyy, nxx = ny + 2 * npad, nx + 2 * npad
    out = np.zeros((nplane, nyy, nxx))
    out[:, npad:-npad, npad:-npad] = cube
    uy = np.linspace(0, nyy - 1, nyy) / nyy
    uy = np.where(uy > 0.5, uy - 1, uy)
    ux = np.linspace(0, nxx - 1, nxx) / nxx
    ux = np.where(ux > 0.5, ux - 1, ux)
    s = np.sinc(ux[None, :] * width) * np.sinc(uy[:, None] * width)
    out = np.real(_ifft2(_fft2(out, extended) * s[None], extended)).astype(np.float64)
    return out[:, npad:-npad, npad:-npad]


def gauss_stamp(n, C):
    X_ = np.linspace((1 - n) / 2.0, (n - 1) / 2.0, n)
    xx, yy = np.meshgrid(X_, X_)
    detC = C[0, 0] * C[1, 1] - C[0, 1] ** 2
    iC = np.array([[C[1, 1], -C[0, 1]], [-C[0, 1], C[0, 0]]]) / detC
    return np.exp(-0.5 * (iC[0, 0] * xx**2 + iC[1, 1] * yy**2) - iC[0, 1] * xx * yy) / (2 * np.pi * np.sqrt(detC))


def gauss_deconv(arr, C, eps, extended=False):
    n = arr.shape[1]
    big = np.zeros((2 * n, 2 * n))
    big[:n, :n] = arr
    u_ = np.linspace(0, 2 * n - 1, 2 * n) / (2 * n)
    u_[n:] = u_[n:] - 1
    u, v = np.meshgrid(u_, u_)
    G = np.exp(-2 * np.pi**2 * (C[0, 0] * u**2 + C[1, 1] * v**2 + 2 * C[0, 1] * u * v))
    return _ifft2(_fft2(big, extended) * (G / (G**2 + eps**2)), extended).real.astype(np.float64)[:n, :n]


def convolve_same(a, b, extended=False):
    """scipy.signal.convolve(a, b, mode="same", method="fft") for two n x n arrays; extended: the same sum by longdouble transforms."""
    if not extended:
        return scipy.signal.convolve(a, b, mode="same", method="fft")
    n = a.shape[0]
    A, B = np.zeros((2 * n, 2 * n)), np.zeros((2 * n, 2 * n))
    A[:n, :n], B[:n, :n] = a, b
    full = scipy.fft.ifft2(scipy.fft.fft2(A.astype(np.clongdouble)) * scipy.fft.fft2(B.astype(np.clongdouble))).real
    o = (n - 1) // 2
    return full[o:o + n, o:o + n].astype(np.float64)


def grid(lorder):
    x, w = roots_legendre(lorder + 1)
    xg, yg = np.meshgrid(x, x)
    xg, yg = xg.flatten(), yg.flatten()
    lpw = np.stack([np.outer(eval_legendre(range(lorder + 1), yg[i]), eval_legendre(range(lorder + 1), xg[i])).flatten() for i in range(len(xg))])
    return xg, yg, np.outer(w, w).flatten(), lpw


def build(psfcube, cov, *, oversamp, r_in, r_out, eps, m_trunc=0, smallstamp_size=None, extended=False, points=None):
    """splitpsf.py:219-284 on the cube as the constructor leaves it, with Cov [npoly, 2, 2] given.  ``points``: only these grid points
    (K_real, zeta_real and locLRP rows of the others stay zero, K_Legendre is then partial)."""
    npoly, n, _ = psfcube.shape
    lorder = int(round(np.sqrt(npoly))) - 1
    ns = n if smallstamp_size is None else smallstamp_size
    W = window_2d(n, oversamp * r_in, oversamp * r_out)
    ntrim = (n - ns) // 2
    small = W[None] * psfcube
    if ntrim > 0:
        small = small[:, ntrim:-ntrim, ntrim:-ntrim]
    resid = psfcube * (1 - W)[None] * truncate_2d(n, m_trunc)[None]
    xg, yg, wg, lpw = grid(lorder)
    KL, Kr, ze, loc = (np.zeros((npoly, n, n)) for _ in range(4))
    for i in (range(npoly) if points is None else points):
        loc[i] = np.einsum("a,aij->ij", lpw[i], resid)
        Kr[i] = gauss_deconv(loc[i], cov[i], eps, extended)
        ze[i] = loc[i] - convolve_same(Kr[i], gauss_stamp(n, cov[i]), extended)
        KL += wg[i] * np.tensordot(lpw[i], Kr[i], axes=0)
    l_ = np.arange(lorder + 1) + 0.5
    KL = KL * np.outer(l_, l_).flatten()[:, None, None]
    return {"smallpsf": small, "K_Legendre": KL, "K_real": Kr, "zeta_real": ze, "locLRP": loc}


def bound(ref_err, ref):
    """The distance the device result may have from the reference: ten times the reference's own distance from the extended-precision
    evaluation, or the table tolerance of tests/parity.py (2e-13 of the maximum) where that is larger."""
    return max(10.0 * float(ref_err), 2e-13 * float(np.max(np.abs(ref))))
