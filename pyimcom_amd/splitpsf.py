"""Short-range PSFs and long-range kernels from Legendre PSF cubes on the device: the numerical content of ``pyimcom.splitpsf.splitpsf``
(reference src/pyimcom/splitpsf/splitpsf.py): ``SplitPSF`` (187-284) and the per-SCA loop of ``split_psf_to_fits`` (333-377) without FITS.

The device does the passes over the cube (csrc/splitpsf.hip): the tophat filter of the constructor, the windows and the split, and per
Gauss-Legendre grid point the Legendre combination, the Gaussian deconvolution, the error map zeta and the update of ``K_Legendre``,
batched over grid points and SCAs.  The host keeps what is small: the Gauss-Legendre nodes and weights and the Legendre values
(``numpy.polynomial.legendre``), the Jacobian of the WCS and the covariances.

A numpy cube gives numpy attributes; a float64 torch tensor on the device gives torch attributes with no host round trip.  The float32
``K_Legendre`` of ``split_cubes`` is what ``pyimcom_amd.imsubtract.LongRangeSubtractor`` takes.  INTEGRATION.md, seam 7."""

import numpy as np

from ._dev import bound_context, is_torch, staged
from ._lib import MEM_DEVICE, check, lib, ptr

__all__ = ["SplitPSF", "split_cubes", "gauss_legendre_grid", "legendre_weights", "jacobian", "covariances", "routes", "ROUTE_LINES", "ROUTE_DENSE"]

FILL = 0.8  # share of the free device memory a chunk plan may use
ROUTE_LINES, ROUTE_DENSE = 1, 2  # how a transform side is served (csrc/splitpsf.hip): wave-per-line butterflies, dense DFT on the MFMA engine
DEFAULTS = {"ref_pixscale": 0.11, "oversamp": 8, "tophat_in": False, "nside": 4088, "r_in": 4.0, "r_out": 9.0, "sigmaGamma": 1.0, "eps": 0.02,
            "m_trunc": 0}  # splitpsf.py:190-200; smallstamp_size defaults to the side of the cube


def gauss_legendre_grid(lorder):
    """splitpsf.py:239-243: (xg, yg, wg) of the (lorder + 1)^2 grid points, i = iy * (lorder + 1) + ix."""
    x, w = np.polynomial.legendre.leggauss(lorder + 1)
    xg, yg = np.meshgrid(x, x)
    return xg.flatten(), yg.flatten(), np.outer(w, w).flatten()


def legendre_weights(lorder, xg, yg):
    """splitpsf.py:263-265 for every grid point: lpw [npoly, npoly], row i = outer(P(y_i), P(x_i)).flatten() (plane a = l_y (lorder + 1) + l_x)."""
    px = np.polynomial.legendre.legvander(np.asarray(xg, dtype=np.float64), lorder)
    py = np.polynomial.legendre.legvander(np.asarray(yg, dtype=np.float64), lorder)
    return np.ascontiguousarray((py[:, :, None] * px[:, None, :]).reshape(len(px), -1))


def jacobian(wcs_, x, y):
    """wcsutil.py:637-685 (local_partial_pixel_derivatives2): the 2 x 2 Jacobian (0 -> West, 1 -> North, degrees per pixel) at pixel (x, y)
    from nine ``all_pix2world`` positions and the 4-point derivative formula.  ``wcs_``: any object with ``all_pix2world(xy [k, 2], 0)``."""
    dx = np.array([0, 1, -1, 3, -3, 0, 0, 0, 0])
    dy = np.array([0, 0, 0, 0, 0, 1, -1, 3, -3])
    degree = np.pi / 180.0
    world = np.asarray(wcs_.all_pix2world(np.vstack((x + dx, y + dy)).T, 0))
    ra, dec = world[:, 0] * degree, world[:, 1] * degree
    p = np.zeros((2, 9))
    p[0] = np.cos(dec) * np.sin(ra[0] - ra)
    p[1] = np.sin(dec) * np.cos(dec[0]) - np.cos(dec) * np.sin(dec[0]) * np.cos(ra[0] - ra)
    jac = np.zeros((2, 2))
    for j in (0, 1):
        s = p[:, 1 + 4 * j:5 + 4 * j]
        jac[:, j] = (27 * (s[:, 0] - s[:, 1]) - (s[:, 2] - s[:, 3])) / 48.0
    return jac / degree


def covariances(wcs_, lorder, *, oversamp, sigmaGamma, nside, ref_pixscale):
    """splitpsf.py:246, 254-260: Cov [npoly, 2, 2] of the target Gaussian at the grid points, in oversampled pixels; the identity times
    (oversamp sigmaGamma)^2 without a WCS."""
    xg, yg, _ = gauss_legendre_grid(lorder)
    var_ref = (oversamp * sigmaGamma) ** 2
    cov = np.zeros((len(xg), 2, 2))
    for i in range(len(xg)):
        if wcs_ is None:
            cov[i] = var_ref * np.identity(2)
        else:
            jac = jacobian(wcs_, nside / 2.0 * (1 + xg[i]), nside / 2.0 * (1 + yg[i]))
            cov[i] = var_ref * np.linalg.inv(jac.T @ jac) * (ref_pixscale / 3600) ** 2
    return cov


def _sizes(n, npoly, width, nsca=1, npts=1):
    out = np.zeros(6, dtype=np.int64)
    check(lib.imcom_splitpsf_sizes(int(n), int(npoly), float(width), int(nsca), int(npts), ptr(out)))
    return out


def routes(n, oversamp=8):
    """(route of the tophat filter's transforms of side n + 2 npad, route of the 2n transforms of ``build``): ROUTE_LINES, ROUTE_DENSE or 0
    (a side this build does not transform: the call raises)."""
    sz = _sizes(n, 1, oversamp)
    return int(sz[2]), int(sz[3])


def _plan_points(n, npoly, nsca, free_bytes, resident_per_sca):
    """(SCAs per call, grid points per call) from exact byte counts: all the grid points of as many SCAs as fit, or -- when one SCA does
    not fit -- as many grid points of one SCA as do."""
    room = int(FILL * free_bytes)
    for c in range(nsca, 0, -1):
        if c * resident_per_sca + int(_sizes(n, npoly, 1.0, c, npoly)[5]) <= room:
            return c, npoly
    for k in range(npoly - 1, 0, -1):
        if resident_per_sca + int(_sizes(n, npoly, 1.0, 1, k)[5]) <= room:
            return 1, k
    raise MemoryError(f"splitpsf: {free_bytes} bytes free on the device, one grid point of one SCA of side {n} needs "
                      f"{resident_per_sca + int(_sizes(n, npoly, 1.0, 1, 1)[5])}")


def _lorder(npoly):
    lorder = 0
    while (lorder + 1) ** 2 < npoly:
        lorder += 1
    return lorder


class SplitPSF:
    """``SplitPSF(psfcube, wcs_, pars)`` with the reference's parameters and defaults (splitpsf.py:187-217); ``build()`` leaves ``smallpsf``
    [npoly, ns, ns], ``K_Legendre``, ``K_real``, ``zeta_real`` [npoly, n, n] and ``Cov`` [npoly, 2, 2] (float64), and ``maxzeta`` =
    max |zeta_real|.  ``cov=`` [npoly, 2, 2] may be given instead of a WCS."""

    def __init__(self, psfcube, wcs_, pars, *, cov=None, device="cuda:0", ctx=None):
        import torch

        pars = dict(pars or {})
        for k, v in DEFAULTS.items():
            setattr(self, k, pars.get(k, v))
        shape = tuple(psfcube.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError("psfcube is [npoly, n, n]")
        self.largestamp_size = int(shape[1])
        self.smallstamp_size = int(pars.get("smallstamp_size", self.largestamp_size))
        self.wcs_ = wcs_
        self.npoly = int(shape[0])
        self.lorder = _lorder(self.npoly)
        if self.smallstamp_size % 2 != 0 or self.largestamp_size % 2 != 0:
            raise ValueError("SplitPSF requires even dimension")
        if (self.lorder + 1) ** 2 != self.npoly:
            raise ValueError("SplitPSF Legendre polynomial dimension error")
        if self.smallstamp_size > self.largestamp_size or self.smallstamp_size < 2:
            raise ValueError(f"smallstamp_size={self.smallstamp_size} for a cube of side {self.largestamp_size}")
        self._torch_in = is_torch(psfcube)
        if self._torch_in:
            if not (psfcube.dtype == torch.float64 and psfcube.is_cuda):
                raise ValueError("a torch psfcube must be a float64 tensor on the device")
            self.dev = psfcube.device
            cube = psfcube.contiguous()
        else:
            self.dev = torch.device(device)
            cube = staged(psfcube, self.dev, astype=np.float64)
        self.ctx = bound_context(self.dev, ctx)
        self._cov_in = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(self.npoly, 2, 2)
        n = self.largestamp_size
        if self.tophat_in:
            self._cube = cube.clone() if self._torch_in else cube  # (np.copy of the reference)
        else:
            self._cube = torch.empty_like(cube)
            check(lib.imcom_splitpsf_tophat(self.ctx.handle, ptr(cube), self.npoly, n, float(self.oversamp), ptr(self._cube), MEM_DEVICE))
            torch.cuda.current_stream(self.dev).synchronize()  # `cube` may be dropped on return
        self.psfcube = self._cube if self._torch_in else self._cube.cpu().numpy()

    def _out(self, t):
        return t if self._torch_in else t.cpu().numpy()

    def build(self, keep=("K_real", "zeta_real"), points_per_call=None):
        """splitpsf.py:219-284.  ``keep``: which of the per-grid-point stacks ``K_real`` and ``zeta_real`` to materialise (a production
        caller writes neither); ``maxzeta`` is set either way.  ``points_per_call``: grid points per library call instead of the plan's
        (the result does not depend on it, bit for bit)."""
        import torch

        from .stamps import free_device_bytes

        n, ns, npoly, dev = self.largestamp_size, self.smallstamp_size, self.npoly, self.dev
        unknown = set(keep) - {"K_real", "zeta_real"}
        if unknown:
            raise ValueError(f"keep: {sorted(unknown)}")
        xg, yg, wg = gauss_legendre_grid(self.lorder)
        lpw = legendre_weights(self.lorder, xg, yg)
        self.Cov = self._cov_in if self._cov_in is not None else covariances(
            self.wcs_, self.lorder, oversamp=self.oversamp, sigmaGamma=self.sigmaGamma, nside=self.nside, ref_pixscale=self.ref_pixscale)
        cov = np.ascontiguousarray(self.Cov, dtype=np.float64)
        f64 = dict(dtype=torch.float64, device=dev)
        small = torch.empty((npoly, ns, ns), **f64)
        resid = torch.empty((npoly, n, n), **f64)
        KL = torch.empty((npoly, n, n), **f64)
        kreal = torch.empty((npoly, n, n), **f64) if "K_real" in keep else None
        zeta = torch.empty((npoly, n, n), **f64) if "zeta_real" in keep else None
        zmax = torch.zeros(1, **f64)
        bound_context(ctx=self.ctx)
        h = self.ctx.handle
        check(lib.imcom_splitpsf_split(h, ptr(self._cube), npoly, n, ns, float(self.oversamp * self.r_in), float(self.oversamp * self.r_out),
                                       int(self.m_trunc), ptr(small), ptr(resid), MEM_DEVICE))
        step = int(points_per_call) if points_per_call else _plan_points(n, npoly, 1, free_device_bytes(dev), 0)[1]
        for i0 in range(0, npoly, step):
            k = min(step, npoly - i0)
            check(lib.imcom_splitpsf_points(h, ptr(resid), 1, npoly, n, i0, k, ptr(lpw), ptr(wg), ptr(cov), float(self.eps), ptr(KL),
                                            None if kreal is None else ptr(kreal[i0:i0 + k]), None if zeta is None else ptr(zeta[i0:i0 + k]),
                                            ptr(zmax), MEM_DEVICE))
        torch.cuda.current_stream(dev).synchronize()  # `resid` goes back to the allocator
        self.smallpsf, self.K_Legendre = self._out(small), self._out(KL)
        if kreal is not None:
            self.K_real = self._out(kreal)
        if zeta is not None:
            self.zeta_real = self._out(zeta)
        self.maxzeta = float(zmax.item())
        return self


def split_cubes(cubes, wcs_list, pars, *, covs=None, device="cuda:0", ctx=None, sca_per_call=None, points_per_call=None):
    """The arithmetic of the loop of ``split_psf_to_fits`` (splitpsf.py:333-377) for the SCAs of one exposure in batched calls.  ``cubes``
    [nsca, npoly, n, n] float64 (numpy, or a torch tensor on the device); ``wcs_list``: one WCS or None per SCA (None: no distortion,
    TRUEWCS False); ``covs`` [nsca, npoly, 2, 2] instead of the WCSs.  Returns a dict: ``smallpsf`` [nsca, npoly, ns, ns] and
    ``K_Legendre`` [nsca, npoly, n, n] as float32 (350, 356), ``MAXZETA``, ``KINT``, ``K2INT`` [nsca] float64 (365-370, sums over the float64
    ``K_Legendre[0]``) and ``TRUEWCS`` [nsca] bool.  SCAs (and, if one SCA does not fit, grid points) are chunked from the free device
    memory by exact byte counts; the result does not depend on the chunking."""
    import torch

    from .stamps import free_device_bytes

    pars = dict(pars or {})
    P = {k: pars.get(k, v) for k, v in DEFAULTS.items()}
    torch_in = is_torch(cubes)
    shape = tuple(cubes.shape)
    if len(shape) != 4 or shape[2] != shape[3]:
        raise ValueError("cubes is [nsca, npoly, n, n]")
    nsca, npoly, n = int(shape[0]), int(shape[1]), int(shape[2])
    ns = int(pars.get("smallstamp_size", n))
    lorder = _lorder(npoly)
    if ns % 2 != 0 or n % 2 != 0:
        raise ValueError("SplitPSF requires even dimension")
    if (lorder + 1) ** 2 != npoly:
        raise ValueError("SplitPSF Legendre polynomial dimension error")
    if ns > n or ns < 2:
        raise ValueError(f"smallstamp_size={ns} for a cube of side {n}")
    if wcs_list is None:
        wcs_list = [None] * nsca
    if len(wcs_list) != nsca:
        raise ValueError(f"{len(wcs_list)} WCSs for {nsca} SCAs")
    if torch_in:
        if not (cubes.dtype == torch.float64 and cubes.is_cuda):
            raise ValueError("torch cubes must be a float64 tensor on the device")
        dev = cubes.device
    else:
        dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    s = P["oversamp"]
    xg, yg, wg = gauss_legendre_grid(lorder)
    lpw = legendre_weights(lorder, xg, yg)
    if covs is not None:
        cov = np.ascontiguousarray(covs, dtype=np.float64).reshape(nsca, npoly, 2, 2)
    else:
        cov = np.stack([covariances(w, lorder, oversamp=s, sigmaGamma=P["sigmaGamma"], nside=P["nside"], ref_pixscale=P["ref_pixscale"])
                        for w in wcs_list])
    f64 = dict(dtype=torch.float64, device=dev)
    out_small = torch.empty((nsca, npoly, ns, ns), dtype=torch.float32, device=dev)
    out_K = torch.empty((nsca, npoly, n, n), dtype=torch.float32, device=dev)
    zmax = torch.zeros(nsca, **f64)
    kint = torch.zeros(nsca, **f64)
    k2int = torch.zeros(nsca, **f64)
    plane = 8 * npoly * n * n
    resident = 3 * plane + 8 * npoly * ns * ns + (0 if torch_in else plane)  # per SCA of a chunk: filtered cube, resid, K_Legendre, smallpsf (+ upload)
    if sca_per_call or points_per_call:
        chunk, step = int(sca_per_call or 1), int(points_per_call or npoly)
    else:
        chunk, step = _plan_points(n, npoly, nsca, free_device_bytes(dev) - int(_sizes(n, npoly, s)[4]), resident)
    if step < npoly:
        chunk = 1
    h = ctx.handle
    for s0 in range(0, nsca, chunk):
        c = min(chunk, nsca - s0)
        part = cubes[s0:s0 + c]
        cube = part.contiguous() if torch_in else staged(part, dev, astype=np.float64)
        if P["tophat_in"]:
            filt = cube
        else:
            filt = torch.empty_like(cube)
            for j in range(c):  # one call per SCA: the filter pairs the planes of ONE cube
                check(lib.imcom_splitpsf_tophat(h, ptr(cube[j]), npoly, n, float(s), ptr(filt[j]), MEM_DEVICE))
        small = torch.empty((c, npoly, ns, ns), **f64)
        resid = torch.empty((c, npoly, n, n), **f64)
        KL = torch.empty((c, npoly, n, n), **f64)
        for j in range(c):
            check(lib.imcom_splitpsf_split(h, ptr(filt[j]), npoly, n, ns, float(s * P["r_in"]), float(s * P["r_out"]), int(P["m_trunc"]), ptr(small[j]),
                                           ptr(resid[j]), MEM_DEVICE))
        for i0 in range(0, npoly, step):
            k = min(step, npoly - i0)
            check(lib.imcom_splitpsf_points(h, ptr(resid), c, npoly, n, i0, k, ptr(lpw), ptr(wg), ptr(np.ascontiguousarray(cov[s0:s0 + c])),
                                            float(P["eps"]), ptr(KL), None, None, ptr(zmax[s0:s0 + c]), MEM_DEVICE))
        out_small[s0:s0 + c] = small
        out_K[s0:s0 + c] = KL
        kint[s0:s0 + c] = KL[:, 0].sum(dim=(1, 2)) / s**2
        k2int[s0:s0 + c] = (KL[:, 0] ** 2).sum(dim=(1, 2)) / s**2
        torch.cuda.current_stream(dev).synchronize()  # the chunk's tensors go back to the allocator before the next one is cut
        del cube, filt, small, resid, KL
    conv = (lambda t: t) if torch_in else (lambda t: t.cpu().numpy())
    return {"smallpsf": conv(out_small), "K_Legendre": conv(out_K), "MAXZETA": conv(zmax), "KINT": conv(kint), "K2INT": conv(k2int),
            "TRUEWCS": np.array([w is not None for w in wcs_list], dtype=np.bool_)}
