"""A vectorised numpy restatement of the injected star-grid layer (reference src/pyimcom/layer.py:792-854 with the cube PSFs of
coadd.py:476-510, 624-640 and the D5512 interpolator of routine.py:29-181): what pyimcom_amd.inject is checked against at sizes the
reference's own loop cannot reach in a test.  It is pinned to the reference's outputs in tests/golden/inject.npz
(tests/test_inject_host.py).  Host numpy only; nothing here is imported by the package."""

import numpy as np

PAD = 6  # layer.py:822

# routine.py:29-122: taps k and 9 - k are even(fh^2) +/- odd(fh^2) fh, Horner in fh^2
_EVEN = np.array([
    [+1.651881673372979740e-05, -3.145538007199505447e-04, +1.793518183780194427e-03, -2.904014557029917318e-03, +6.187591260980151433e-04],
    [-1.146756217210629335e-04, +2.883845374976550142e-03, -1.857047531896089884e-02, +3.147734488597204311e-02, -6.753293626461192439e-03],
    [+3.256838096371517067e-04, -9.702063770653997568e-03, +8.678848026470635524e-02, -1.659182651092198924e-01, +3.620560878249733799e-02],
    [-4.541830837949564726e-04, +1.494862093737218955e-02, -1.668775957435094937e-01, +5.879306056792649171e-01, -1.367845996704077915e-01],
    [+2.266560930061513573e-04, -7.815848920941316502e-03, +9.686607348538181506e-02, -4.505856722239036105e-01, +6.067135256905490381e-01],
])
_ODD = np.array([
    [-3.486978652054735998e-06, +6.753750285320532433e-05, -3.871378836550175566e-04, +6.279918076641771273e-04, -1.338434614116611838e-04],
    [+3.121412120355294799e-05, -8.040343683015897672e-04, +5.209574765466357636e-03, -8.847326408846412429e-03, +1.898674086370833597e-03],
    [-1.243658986204533102e-04, +3.804930695189636097e-03, -3.434861846914529643e-02, +6.581033749134083954e-02, -1.436476114189205733e-02],
    [+2.894406669584551734e-04, -9.794291009695265532e-03, +1.104231510875857830e-01, -3.906954914039130755e-01, +9.092432925988773451e-02],
    [-4.336085507644610966e-04, +1.537862263741893339e-02, -1.925091434770601628e-01, +8.993141455798455697e-01, -1.213035309579723942e+00],
])


def getw(fh):
    """D5512 weights [..., 10] for fh = frac - 1/2 (routine.py:29-122)."""
    fh = np.asarray(fh, dtype=np.float64)
    fh2 = fh * fh
    w = np.empty(fh.shape + (10,))
    for k in range(5):
        e, o = np.full(fh.shape, _EVEN[k][0]), np.full(fh.shape, _ODD[k][0])
        for c in range(1, 5):
            e = e * fh2 + _EVEN[k][c]
            o = o * fh2 + _ODD[k][c]
        o = o * fh
        w[..., k] = e + o
        w[..., 9 - k] = e - o
    return w


def weight_gain(nfh=20001):
    """max over fh of sum_k |w_k(fh)|: the factor by which one axis of the interpolation can amplify an error of its input."""
    return float(np.abs(getw(np.linspace(-0.5, 0.5, nfh))).sum(axis=-1).max())


def legendre_values(porder, x):
    """P_0 .. P_porder at x [...], by the three-term recurrence -> [..., porder + 1]."""
    x = np.asarray(x, dtype=np.float64)
    P = np.ones(x.shape + (porder + 1,))
    if porder >= 1:
        P[..., 1] = x
    for m in range(2, porder + 1):
        P[..., m] = ((2 * m - 1) * x * P[..., m - 1] - (m - 1) * P[..., m - 2]) / m
    return P


def lpoly_arr(porder, u, v):
    """InImage.LPolyArr (coadd.py:476-510) for arrays of positions: [S, (porder + 1)^2], x order fastest."""
    ua, va = legendre_values(porder, np.atleast_1d(u)), legendre_values(porder, np.atleast_1d(v))
    return (va[:, :, None] * ua[:, None, :]).reshape(ua.shape[0], -1)


def pad_width(tophatwidth, gaussiansigma):
    npad = int(np.ceil(tophatwidth + 6 * gaussiansigma + 1))
    return npad + (4 - npad) % 4


def smooth_and_pad(img, tophatwidth=0.0, gaussiansigma=0.0):
    """InImage.smooth_and_pad (coadd.py:433-474) of an image or a stack [..., ny, nx]."""
    img = np.asarray(img, dtype=np.float64)
    npad = pad_width(tophatwidth, gaussiansigma)
    big = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(npad, npad), (npad, npad)])
    nyy, nxx = big.shape[-2:]
    uy, ux = np.fft.fftfreq(nyy), np.fft.fftfreq(nxx)
    if nyy % 2 == 0:
        uy[nyy // 2] = 0.5  # the reference keeps u = 1/2 positive; the filter is even, so only the convention differs
    if nxx % 2 == 0:
        ux[nxx // 2] = 0.5
    filt = (np.sinc(ux[None, :] * tophatwidth) * np.sinc(uy[:, None] * tophatwidth)
            * np.exp(-2.0 * np.pi**2 * gaussiansigma**2 * (ux[None, :] ** 2 + uy[:, None] ** 2)))
    return np.real(np.fft.ifft2(np.fft.fft2(big) * filt))


def psf_from_cube(cube, lpoly, tophatwidth, gaussiansigma=0.0, scale=1.0):
    """coadd.py:624-640 per star, literally: contract, then smear -> [S, ny + 2 npad, nx + 2 npad]."""
    return scale * smooth_and_pad(np.einsum("sa,aij->sij", np.asarray(lpoly, dtype=np.float64), cube), tophatwidth, gaussiansigma)


def box(pos, d, nside):
    """layer.py:827-830 along one axis for arrays of positions: (lo, hi) of the clipped box (int() truncates towards zero)."""
    ip = np.trunc(np.asarray(pos, dtype=np.float64)).astype(np.int64)
    return np.maximum(0, ip - d), np.minimum(nside, ip + d)


def on_chip(xsca, ysca, nside, d=64):
    """Stars the reference draws (layer.py:831-834): both clipped box sides at least one pixel."""
    x0, x1 = box(xsca, d, nside)
    y0, y1 = box(ysca, d, nside)
    return (x1 - x0 >= 1) & (y1 - y0 >= 1)


def _axis(pos, n, lo, hi, oversamp):
    """Pixels lo..hi-1 of one star along one axis: (pixels on the grid, their first tap in the unpadded PSF, weights [*, 10])."""
    pix = np.arange(lo, hi)
    X = oversamp * (pix - pos) + (n - 1) / 2.0 + PAD
    xi = X.astype(np.int32)
    ok = (xi >= 4) & (xi < n + 2 * PAD - 5)
    pix, X, xi = pix[ok], X[ok], xi[ok]
    return pix, xi - 4, getw(X - xi - 0.5)


def draw_stars(psfs, xsca, ysca, nside, oversamp, d=64, out=None):
    """layer.py:825-852: the stars in ascending order, each as two separable weight matrices applied to its padded PSF
    (x taps inside, y taps outside, routine.py:174-181)."""
    image = np.zeros((nside, nside)) if out is None else out
    psfs = np.asarray(psfs, dtype=np.float64)
    if psfs.ndim == 2:
        psfs = np.broadcast_to(psfs, (len(xsca),) + psfs.shape)
    keep = on_chip(xsca, ysca, nside, d)
    x0, x1 = box(xsca, d, nside)
    y0, y1 = box(ysca, d, nside)
    tap = np.arange(10)
    for s in np.nonzero(keep)[0]:
        P = np.pad(psfs[s], PAD)
        ny, nx = psfs[s].shape
        px_, cx, wx = _axis(xsca[s], nx, x0[s], x1[s], oversamp)
        py_, cy, wy = _axis(ysca[s], ny, y0[s], y1[s], oversamp)
        if px_.size == 0 or py_.size == 0:
            continue
        strips = np.einsum("yixj,xj->yix", P[(cy[:, None] + tap)[:, :, None, None], (cx[:, None] + tap)[None, None, :, :]], wx)
        val = np.einsum("yix,yi->yx", strips, wy)
        image[np.ix_(py_, px_)] += val * oversamp**2
    return image


def star_image(cube, lpoly, xsca, ysca, nside, oversamp, tophatwidth, scale=1.0, d=64):
    """make_image_from_grid after generate_star_grid with cube PSFs; stars off the chip get no PSF."""
    keep = on_chip(xsca, ysca, nside, d)
    psfs = psf_from_cube(cube, np.asarray(lpoly)[keep], tophatwidth, 0.0, scale)
    return draw_stars(psfs, np.asarray(xsca)[keep], np.asarray(ysca)[keep], nside, oversamp, d)
