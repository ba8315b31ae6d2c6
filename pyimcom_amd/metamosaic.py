"""The metadetection mosaic on the device: ``pyimcom.meta.distortimage.MetaMosaic`` (reference src/pyimcom/meta/distortimage.py) without
FITS and without astropy.  The binding (seam 19):

    m = pyimcom_amd.metamosaic.DeviceMetaMosaic(cfg, ix, iy, nlayer, np.float32, extpix=200, stem=stem)
    for dx, dy, in_x, in_y, *_ in m.windows:                       # the blocks the reference's constructor reads (146-207)
        with ReadFile(name(in_x, in_y)) as f:
            m.add_block(dx, dy, f["PRIMARY"].data[0], f["FIDELITY"].data[0], f["SIGMA"].data[0],
                        HDU_to_bels(f["FIDELITY"]), HDU_to_bels(f["SIGMA"]))
    m.mask_fidelity_cut(40.0); m.mask_caps(ra, dec, radius)
    im = m.shearimage(N, jac=..., psfgrow=1.02)                    # the reference's dict; image and mask are device tensors

The four arrays (``in_image`` [nlayer, Nside, Nside], ``in_fidelity`` and ``in_noise`` float32 in dB, ``in_mask`` bool) are device tensors
from the first block on; a block's layers may come from the host, from the device (``BlockMaps.out_map[0]``) or I24-compressed
(``add_block_compressed``).  csrc/ginterp.hip holds the kernels (one launch a block; the mask cuts; the circles of ``mask_caps`` as one
flat index space over all boxes), csrc/mosaic_core.h the index maps, the float32 dB arithmetic, the boxes and the predicate.

``block_windows``, ``mosaic_header``, ``shear_geometry`` and ``orig_geometry`` restate the reference's integer and small-matrix statements
in numpy and touch no device.  ``cfg_like`` is anything with the attributes (or keys) ``n1, n2, postage_pad, nblock, dtheta, ra, dec,
lonpole, outpsf, sigmatarget, extrainput`` of ``pyimcom.config.Config`` (``Nside`` = n1 n2 if absent).

Differences from the reference, all at the edges: ``in_mask`` starts all-masked and a block's launch writes ``in_fidelity == 0`` on its
window (the reference forms ``in_fidelity == 0`` once after all blocks: the same array, but a block added after a mask method overwrites
the mask of its window); a catalogue position that is not finite raises ``ValueError`` before any pixel is set (the reference's
``int(np.floor(nan))`` raises on reaching the object); ``im["wcs"]`` is the header dict the reference hands to ``astropy.wcs.WCS`` and
``im["device_wcs"]`` a ``DeviceWCS`` of it.  FITS, ``ReadFile``, ``Config`` parsing, ``to_file`` and ``shearimage_to_fits`` stay the
reference's; ``to_host()`` gives the arrays ``to_file`` writes."""

import numpy as np

from . import ginterp
from ._dev import DEVICE, bound_context, np_dtype, staged
from ._lib import check, lib, ptr
from .wcs import DeviceWCS

__all__ = ["DeviceMetaMosaic", "block_windows", "mosaic_header", "shear_geometry", "orig_geometry", "PIXSCALE_NATIVE", "CODE_TYPES"]

PIXSCALE_NATIVE = 0.11 * (np.pi / 180.0 / 60.0 / 60.0)  # Settings.pixscale_native (config.py:85-97), radians
CODE_TYPES = {"uint8": 0, "uint16": 1, "int16": 2}        # the `type` of imcom_mosaic_paste's coded maps


def _c(cfg, name):
    if isinstance(cfg, dict):
        if name == "Nside" and name not in cfg:
            return cfg["n1"] * cfg["n2"]
        return cfg[name]
    if name == "Nside" and not hasattr(cfg, name):
        return cfg.n1 * cfg.n2
    return getattr(cfg, name)


def block_windows(cfg_like, ix, iy, bbox=None, extpix=None):
    """distortimage.py:120-171: (trunc, Nside, windows), one window per block file the constructor reads, in its order:
    (dx, dy, in_x, in_y, symin, symax, sxmin, sxmax, cx, cy) -- rows symin:symax and columns sxmin:sxmax of block (in_x, in_y) go to the
    rows symin + cy : symax + cy and the columns sxmin + cx : sxmax + cx of the mosaic."""
    n1, n2, pad, nblock = (int(_c(cfg_like, k)) for k in ("n1", "n2", "postage_pad", "nblock"))
    if bbox is None:
        xmin_ = ymin_ = 0
        xmax_ = ymax_ = nblock
    else:
        xmin_, xmax_, ymin_, ymax_ = bbox[0], bbox[1], bbox[2], bbox[3]
    trunc = 0 if extpix is None else max(n1 * n2 - extpix, 0)
    Nside = 3 * n1 * n2 - 2 * trunc
    xpad = [ix == 0, ix == nblock - 1]
    ypad = [iy == 0, iy == nblock - 1]
    block_min, block_max = -1, 2
    if (extpix is not None) and extpix <= 0:
        block_min, block_max = 0, 1
    windows = []
    for dx in range(block_min, block_max):
        cx = n1 * n2 * (1 + dx) - pad * n2 - trunc
        sxmin = pad * n2
        sxmax = sxmin + n1 * n2
        if xpad[0]:
            sxmin -= pad * n2
        if xpad[1]:
            sxmax += pad * n2
        if cx + sxmin < 0:
            sxmin = -cx
        if cx + sxmax > Nside:
            sxmax = Nside - cx
        for dy in range(block_min, block_max):
            cy = n1 * n2 * (1 + dy) - pad * n2 - trunc
            symin = pad * n2
            symax = symin + n1 * n2
            if ypad[0]:
                symin -= pad * n2
            if ypad[1]:
                symax += pad * n2
            if cy + symin < 0:
                symin = -cy
            if cy + symax > Nside:
                symax = Nside - cy
            in_x, in_y = ix + dx, iy + dy
            if in_x >= xmin_ and in_x < xmax_ and in_y >= ymin_ and in_y < ymax_:
                windows.append((dx, dy, in_x, in_y, symin, symax, sxmin, sxmax, cx, cy))
    return trunc, Nside, windows


def _stg_header(cfg_like, crpix1, crpix2, N, cd):
    """The dict that 479-497 and 639-657 hand to astropy.wcs.WCS."""
    return {"CTYPE1": "RA---STG", "CUNIT1": "deg", "CRPIX1": crpix1, "NAXIS1": N, "CTYPE2": "DEC--STG", "CUNIT2": "deg", "CRPIX2": crpix2, "NAXIS2": N,
            "CD1_1": cd[0], "CD1_2": cd[1], "CD2_1": cd[2], "CD2_2": cd[3], "CRVAL1": _c(cfg_like, "ra"), "CRVAL2": _c(cfg_like, "dec"),
            "LONPOLE": _c(cfg_like, "lonpole")}


def mosaic_header(cfg_like, ix, iy, trunc):
    """distortimage.py:212-221 as a header dict (``DeviceWCS.from_header`` takes it)."""
    Nside, nblock, dtheta = _c(cfg_like, "Nside"), _c(cfg_like, "nblock"), _c(cfg_like, "dtheta")
    return {"CTYPE1": "RA---STG", "CTYPE2": "DEC--STG", "CRPIX1": 0.5 - Nside * (ix - 1 - nblock // 2) - trunc, "CRPIX2": 0.5 - Nside * (iy - 1 - nblock // 2) - trunc,
            "CDELT1": -dtheta, "CDELT2": dtheta, "CRVAL1": _c(cfg_like, "ra"), "CRVAL2": _c(cfg_like, "dec"), "LONPOLE": _c(cfg_like, "lonpole")}


def _require_gaussian(cfg_like):
    if _c(cfg_like, "outpsf") != "GAUSSIAN":
        raise ValueError("shearimage: only works on GAUSSIAN, received " + str(_c(cfg_like, "outpsf")))


def shear_geometry(cfg_like, ix, iy, trunc, N, jac=None, psfgrow=1.0, oversamp=1.0, stem=""):
    """distortimage.py:457-509 and 540-583: a dict of ``xref, yref, opos, J, sigma, C``, ``header`` (479-497) and ``pardict`` (557-583 without
    UMAX and SMAX, which the resampler returns)."""
    n1, n2, nblock, dtheta, sigmatarget = (_c(cfg_like, k) for k in ("n1", "n2", "nblock", "dtheta", "sigmatarget"))
    J = np.identity(2) if jac is None else np.asarray(jac)
    J_orig = np.copy(J)
    J = J / oversamp
    scale = dtheta
    Q_orig = np.asarray([nblock / 2 - ix - 0.5, nblock / 2 - iy - 0.5]) * n1 * n2
    Q_new = np.linalg.solve(J, Q_orig)
    xref = np.round(Q_new[0] + 1e-7) + 0.5 + N / 2
    yref = np.round(Q_new[1] + 1e-7) + 0.5 + N / 2
    opos = J @ np.asarray([1 - xref, 1 - yref])
    opos[0] += (nblock / 2 - ix + 1) * n1 * n2 - 0.5 - trunc
    opos[1] += (nblock / 2 - iy + 1) * n1 * n2 - 0.5 - trunc
    header = _stg_header(cfg_like, xref, yref, N, (-J[0, 0] * scale, -J[0, 1] * scale, J[1, 0] * scale, J[1, 1] * scale))
    sigma = sigmatarget * PIXSCALE_NATIVE * (180.0 / np.pi) / dtheta
    dCov = sigma**2 * (psfgrow**2 * J_orig @ J_orig.T - np.identity(2))
    C = [dCov[0, 0], dCov[0, 1], dCov[1, 1]]
    z = J_orig[0, 0] + J_orig[1, 1] + 1j * (J_orig[1, 0] - J_orig[0, 1])
    cpd = np.abs(z)
    apx = np.angle(z)
    z = J_orig[0, 0] - J_orig[1, 1] + 1j * (J_orig[1, 0] + J_orig[0, 1])
    cmd = np.abs(z)
    amx = np.angle(z)
    Eig1 = (cpd + cmd) / 2.0
    Eig2 = (cpd - cmd) / 2.0
    alpha = (apx + amx) / 2.0
    mu = 1.0 / (Eig1 * Eig2)
    eta = -np.log(Eig1 / Eig2)
    eta1 = eta * np.cos(2 * alpha)
    eta2 = eta * np.sin(2 * alpha)
    g1 = np.tanh(eta / 2.0) * np.cos(2 * alpha)
    g2 = np.tanh(eta / 2.0) * np.sin(2 * alpha)
    conv = 1.0 - (Eig1 + Eig2) / 2.0
    pardict = {
        "STEM": (stem, "stem for file name"),
        "BLOCKX": (ix, "x block index"),
        "BLOCKY": (iy, "y block index"),
        "JXX": (J_orig[0, 0], "Jacobian x_in, x_out"),
        "JXY": (J_orig[0, 1], "Jacobian x_in, y_out"),
        "JYX": (J_orig[1, 0], "Jacobian y_in, x_out"),
        "JYY": (J_orig[1, 1], "Jacobian y_in, y_out"),
        "COVXX": (C[0], "smoothing covariance xx"),
        "COVXY": (C[1], "smoothing covariance xy"),
        "COVYY": (C[2], "smoothing covariance yy"),
        "SIGMAOUT": (sigmatarget * PIXSCALE_NATIVE * (180.0 / np.pi) * 3600 * psfgrow, "arcsec"),
        "PIXSCALE": (dtheta * 3600 / oversamp, "arcsec"),
        "OVERSAMP": (oversamp, "oversampling implemented in shearimage"),
        "MU": (mu, "amplification applied"),
        "ETA1": (eta1, "shear component 1"),
        "ETA2": (eta2, "shear component 2"),
        "JROTATE": (apx, "rotation angle, CCW in-->out, radians"),
        "G1": (g1, "reduced shear component 1"),
        "G2": (g2, "reduced shear component 2"),
        "CONV": (conv, "convergence kappa"),
    }
    return {"xref": xref, "yref": yref, "opos": opos, "J": J, "sigma": sigma, "C": C, "header": header, "pardict": pardict}


def orig_geometry(cfg_like, ix, iy, trunc, N=None, stem=""):
    """distortimage.py:617-657 and 673-696: a dict of ``N, xref, yref, opos`` (the integer offset ``opos_`` of 636), ``header`` and
    ``pardict`` (complete: UMAX 0, SMAX 1)."""
    n1, n2, nblock, dtheta, sigmatarget = (_c(cfg_like, k) for k in ("n1", "n2", "nblock", "dtheta", "sigmatarget"))
    if N is None:
        N = n1 * n2
    dshift = (n1 * n2 + N) % 2
    scale = dtheta
    xref = (nblock / 2 - ix - 0.5) * n1 * n2 + (N + dshift + 1) / 2
    yref = (nblock / 2 - iy - 0.5) * n1 * n2 + (N + dshift + 1) / 2
    opos_ = (3 * n1 * n2 - N - dshift) // 2 - trunc
    header = _stg_header(cfg_like, xref, yref, N, (-scale, 0.0, 0.0, scale))
    pardict = {
        "STEM": (stem, "stem for file name"),
        "BLOCKX": (ix, "x block index"),
        "BLOCKY": (iy, "y block index"),
        "UMAX": (0.0, "interp - max leakage (square norm)"),
        "SMAX": (1.0, "interp - max noise (square norm)"),
        "JXX": (1.0, "Jacobian x_in, x_out"),
        "JXY": (0.0, "Jacobian x_in, y_out"),
        "JYX": (0.0, "Jacobian y_in, x_out"),
        "JYY": (1.0, "Jacobian y_in, y_out"),
        "COVXX": (0.0, "smoothing covariance xx"),
        "COVXY": (0.0, "smoothing covariance xy"),
        "COVYY": (0.0, "smoothing covariance yy"),
        "SIGMAOUT": (sigmatarget * PIXSCALE_NATIVE * (180.0 / np.pi) * 3600, "arcsec"),
        "PIXSCALE": (dtheta * 3600, "arcsec"),
        "OVERSAMP": (1.0, "oversampling implemented in shearimage"),
        "MU": (1.0, "amplification applied"),
        "ETA1": (0.0, "shear component 1"),
        "ETA2": (0.0, "shear component 2"),
        "JROTATE": (0.0, "rotation angle, CCW in-->out, radians"),
        "G1": (0.0, "reduced shear component 1"),
        "G2": (0.0, "reduced shear component 2"),
        "CONV": (0.0, "convergence kappa"),
    }
    return {"N": N, "xref": xref, "yref": yref, "opos": opos_, "header": header, "pardict": pardict}


def _layer_list(cfg_like, nlayer, select_layers):
    """526-532 / 659-665: (ul int64, the names of the selected layers)."""
    ul = np.arange(nlayer).astype(np.int64)
    if select_layers is not None:
        ul = np.array(select_layers).astype(np.int64)
    extrainput = _c(cfg_like, "extrainput")
    return ul, [extrainput[ul[i]] for i in range(len(ul))]


class DeviceMetaMosaic:
    """``MetaMosaic`` with its arrays on the device.  ``nlayer`` and ``dtype`` (float32 or float64) are what the reference's constructor
    reads from the first file's ``PRIMARY``; ``windows`` lists the blocks to add (``block_windows``)."""

    def __init__(self, cfg_like, ix, iy, nlayer, dtype=np.float32, bbox=None, extpix=None, device=DEVICE, ctx=None, stem=""):
        import torch

        self.cfg, self.ix, self.iy, self.nlayer, self.stem = cfg_like, int(ix), int(iy), int(nlayer), stem
        self.im_dtype = np.dtype(dtype)
        if self.im_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"DeviceMetaMosaic: layers of dtype {self.im_dtype} (float32 and float64 are supported)")
        if self.nlayer < 1:
            raise ValueError(f"DeviceMetaMosaic: {nlayer} layers")
        self.trunc, self.Nside, self.windows = block_windows(cfg_like, self.ix, self.iy, bbox, extpix)
        self._window = {(w[0], w[1]): w for w in self.windows}
        self.device = torch.device(device)
        self._ctx = ctx
        ns = self.Nside
        tdt = torch.float32 if self.im_dtype == np.float32 else torch.float64
        self.in_image = torch.zeros((self.nlayer, ns, ns), dtype=tdt, device=self.device)
        self.in_fidelity = torch.zeros((ns, ns), dtype=torch.float32, device=self.device)
        self.in_noise = torch.zeros((ns, ns), dtype=torch.float32, device=self.device)
        self.in_mask = torch.ones((ns, ns), dtype=torch.bool, device=self.device)  # (in_fidelity == 0 where no block has been pasted)
        self.header = mosaic_header(cfg_like, self.ix, self.iy, self.trunc)
        self.wcs = DeviceWCS.from_header(self.header, array_shape=(ns, ns))

    def _context(self):
        return bound_context(self.device, self._ctx)

    # ---- blocks ----
    def _on_device(self, a, what, dtypes):
        """A tensor of ``a`` on the mosaic's device with unit stride along its rows, read in place when it already is one."""
        t = staged(a, self.device, dtypes, f"DeviceMetaMosaic: {what} of dtype {{name}} (supported: {', '.join(dtypes)})", layout="rows")
        return t, np_dtype(t).name

    def paste(self, window, primary, fidelity, sigma, fid_bels, sig_bels):
        """The launch of ``add_block`` with an explicit ``window`` = (symin, symax, sxmin, sxmax, cx, cy)."""
        symin, symax, sxmin, sxmax, cx, cy = (int(v) for v in window)
        p, pname = self._on_device(primary, "PRIMARY", ("float32", "float64"))
        if np.dtype(pname) != self.im_dtype:
            raise TypeError(f"DeviceMetaMosaic: PRIMARY of dtype {pname} for a mosaic of {self.im_dtype}")
        if p.dim() != 3 or p.shape[0] != self.nlayer:
            raise ValueError(f"DeviceMetaMosaic: PRIMARY of shape {tuple(p.shape)}, expected ({self.nlayer}, ny, nx)")
        f, fname = self._on_device(fidelity, "FIDELITY", tuple(CODE_TYPES))
        s, sname = self._on_device(sigma, "SIGMA", tuple(CODE_TYPES))
        by, bx = int(p.shape[1]), int(p.shape[2])
        if tuple(f.shape) != (by, bx) or tuple(s.shape) != (by, bx):
            raise ValueError(f"DeviceMetaMosaic: FIDELITY {tuple(f.shape)} and SIGMA {tuple(s.shape)} for layers of {(by, bx)}")
        if p.stride(1) < bx or f.stride(0) < bx or s.stride(0) < bx or p.stride(0) < 0:
            p, f, s = p.contiguous(), f.contiguous(), s.contiguous()
        ctx = self._context()
        check(lib.imcom_mosaic_paste(ctx.handle, ptr(p), int(self.im_dtype == np.float64), p.stride(0) if self.nlayer > 1 else 0, p.stride(1), self.nlayer, by, bx,
                                     ptr(f), CODE_TYPES[fname], f.stride(0), float(fid_bels), ptr(s), CODE_TYPES[sname], s.stride(0), float(sig_bels),
                                     symin, symax, sxmin, sxmax, cy, cx, self.Nside, ptr(self.in_image), ptr(self.in_fidelity), ptr(self.in_noise), ptr(self.in_mask)))

    def _lookup(self, dx, dy):
        w = self._window.get((int(dx), int(dy)))
        if w is None:
            raise ValueError(f"DeviceMetaMosaic: block offset ({dx}, {dy}) is not among the blocks this mosaic reads: {sorted(self._window)}")
        return w[4:]

    def add_block(self, dx, dy, primary, fidelity, sigma, fid_bels, sig_bels):
        """191-207 for the block (ix + dx, iy + dy): ``primary`` [nlayer, ny, nx] (``f["PRIMARY"].data[0]``, or ``BlockMaps.out_map[0]``),
        ``fidelity`` and ``sigma`` the coded maps [ny, nx] (uint8, uint16 or int16), ``fid_bels`` and ``sig_bels`` what ``HDU_to_bels`` gives
        for their HDUs (NaN where it gives NaN).  numpy arrays are uploaded, device tensors read in place."""
        self.paste(self._lookup(dx, dy), primary, fidelity, sigma, fid_bels, sig_bels)

    def add_block_compressed(self, dx, dy, cubes, pars_list, overflows, fidelity, sigma, fid_bels, sig_bels):
        """``add_block`` with I24-compressed layers (``pyimcom_amd.i24.decompress_layers``'s arguments): decoded on the device, no host copy.
        The codec yields float32."""
        from . import i24

        window = self._lookup(dx, dy)
        layers = i24.decompress_layers(cubes, pars_list, overflows, ctx=self._ctx, device=self.device)
        self.paste(window, layers, fidelity, sigma, fid_bels, sig_bels)

    # ---- masks ----
    def _cut(self, mask, mode, values, cut, extra=None):
        """imcom_mosaic_mask_cut on ``mask`` (a bool tensor: one byte a pixel, 0 or 1)."""
        if cut is not None and np.result_type(np.float32, cut) == np.float32:
            cut = np.float32(cut)  # (numpy compares a float32 array with a Python float in float32)
        ctx = self._context()
        check(lib.imcom_mosaic_mask_cut(ctx.handle, ptr(mask), ptr(values), mask.numel(), 0.0 if cut is None else float(cut), mode, ptr(extra)))

    def maskpix(self, extramask):
        """223-240: pixels that are True in ``extramask`` (numpy or tensor, [Nside, Nside]) are masked."""
        e = staged(extramask, self.device) != 0
        if tuple(e.shape) != (self.Nside, self.Nside):
            raise ValueError(f"maskpix: a mask of shape {tuple(e.shape)} for a mosaic of side {self.Nside}")
        self._cut(self.in_mask, 0, None, None, e)

    def mask_fidelity_cut(self, fidelitymin):
        """242-260: ``in_mask |= in_fidelity < fidelitymin`` (a NaN fidelity compares False)."""
        self._cut(self.in_mask, 1, self.in_fidelity, fidelitymin)

    def mask_noise_cut(self, noisemax):
        """262-280: ``in_mask |= in_noise > noisemax``."""
        self._cut(self.in_mask, 2, self.in_noise, noisemax)

    def mask_caps_pixels(self, x, y, r):
        """340-352: the circles of radius ``r`` pixels at the pixel positions (``x``, ``y``) (0-offset), numpy or tensors of one length."""
        import torch

        cols = []
        for v in (x, y, r):
            cols.append(staged(v, self.device, astype=np.float64).reshape(-1))
        n = cols[0].numel()
        if cols[1].numel() != n or cols[2].numel() != n:
            raise ValueError(f"mask_caps_pixels: {[c.numel() for c in cols]} positions and radii")
        if n == 0:
            return
        if not bool(torch.isfinite(torch.stack(cols)).all()):
            raise ValueError("mask_caps: cannot convert a position or radius that is not finite to a pixel")
        ctx = self._context()
        check(lib.imcom_mosaic_caps(ctx.handle, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), n, self.Nside, ptr(self.in_mask)))

    def mask_caps(self, ra, dec, radius):
        """282-352: circles of ``radius`` degrees (an array, or one value for all) around the catalogue positions (``ra``, ``dec``) in
        degrees.  The preselection of 314-331 runs in numpy on vectors of catalogue length; the positions come from the device WCS."""
        degree = np.pi / 180.0
        ra = np.array(ra).ravel().astype(np.float64)
        dec = np.array(dec).ravel().astype(np.float64)
        radius = np.array(radius).ravel().astype(np.float64)
        if len(radius) == 1:
            radius = np.zeros_like(ra) + radius[0]
        ns = self.Nside
        ra_ctr, dec_ctr = self.wcs.all_pix2world((ns - 1) / 2, (ns - 1) / 2, 0)
        dx = np.cos(dec * degree) * np.cos((ra - ra_ctr) * degree) - np.cos(dec_ctr * degree)
        dy = np.cos(dec * degree) * np.sin((ra - ra_ctr) * degree)
        dz = np.sin(dec * degree) - np.sin(dec_ctr * degree)
        sep = np.sqrt(dx**2 + dy**2 + dz**2) / degree
        searchrad = 0.75 * ns * _c(self.cfg, "dtheta") + radius
        consider_stars = np.nonzero(sep <= searchrad)
        ra, dec, radius = ra[consider_stars], dec[consider_stars], radius[consider_stars]
        if len(ra) == 0:
            return
        pixcrd2 = self.wcs.all_world2pix(np.vstack((ra, dec)).T, 0)
        self.mask_caps_pixels(pixcrd2[:, 0], pixcrd2[:, 1], radius / _c(self.cfg, "dtheta"))

    # ---- images ----
    def origimage(self, N=None, select_layers=None):
        """595-706: the dict of ``shearimage`` for the centred N x N cut-out (default: one block); ``image`` is a view of ``in_image`` (a
        copy when ``select_layers`` is given, as numpy's fancy index is), ``mask`` a copy."""
        _require_gaussian(self.cfg)
        g = orig_geometry(self.cfg, self.ix, self.iy, self.trunc, N, self.stem)
        N, o = g["N"], g["opos"]
        ul, layerlist = _layer_list(self.cfg, self.nlayer, select_layers)
        n12 = _c(self.cfg, "n1") * _c(self.cfg, "n2")
        if o < 0 or o + N > 3 * n12 - 2 * self.trunc:
            raise ValueError("Requested image size too large (overfills original image)")
        image = self.in_image[:, o:o + N, o:o + N] if select_layers is None else self.in_image[ul.tolist(), o:o + N, o:o + N]
        mask = self.in_mask[o:o + N, o:o + N].clone()
        pardict = g["pardict"]
        return {"image": image, "mask": mask, "wcs": g["header"], "device_wcs": DeviceWCS.from_header(g["header"], array_shape=(N, N)), "pars": pardict,
                "layers": layerlist, "psf_fwhm": np.sqrt(8.0 * np.log(2)) * pardict["SIGMAOUT"][0], "ref": (g["xref"] - 1, g["yref"] - 1)}

    def shearimage(self, N, jac=None, psfgrow=1.0, oversamp=1.0, fidelity_min=None, Rsearch=6.0, select_layers=None, verbose=False):
        """393-593: the sheared, reconvolved N x N image of every (selected) layer and its dict.  The mask of ``fidelity_min`` is formed on
        the device and the resampler (``pyimcom_amd.ginterp.MultiInterp``) reads the resident tensors."""
        _require_gaussian(self.cfg)
        g = shear_geometry(self.cfg, self.ix, self.iy, self.trunc, N, jac, psfgrow, oversamp, self.stem)
        if fidelity_min is not None:
            inmask = self.in_mask.clone()
            self._cut(inmask, 1, self.in_fidelity, fidelity_min)
        else:
            inmask = self.in_mask
        ul, layerlist = _layer_list(self.cfg, self.nlayer, select_layers)
        layers = self.in_image if select_layers is None else self.in_image[ul.tolist()]
        if verbose:
            print("opos", g["opos"], "sigma", g["sigma"], "C", g["C"])
        image, mask, Umax, Smax = ginterp.MultiInterp(layers, inmask, (N, N), g["opos"], g["J"], Rsearch, g["sigma"] * np.sqrt(8 * np.log(2)), g["C"])
        pardict = {}
        for k, v in g["pardict"].items():  # (the reference's key order: UMAX and SMAX after BLOCKY)
            pardict[k] = v
            if k == "BLOCKY":
                pardict["UMAX"] = (Umax, "interp - max leakage (square norm)")
                pardict["SMAX"] = (Smax, "interp - max noise (square norm)")
        return {"image": image, "mask": mask, "wcs": g["header"], "device_wcs": DeviceWCS.from_header(g["header"], array_shape=(N, N)), "pars": pardict,
                "layers": layerlist, "psf_fwhm": np.sqrt(8.0 * np.log(2)) * pardict["SIGMAOUT"][0], "ref": (g["xref"] - 1, g["yref"] - 1)}

    def to_host(self):
        """(in_image, in_fidelity, in_noise, in_mask as uint8): the arrays ``MetaMosaic.to_file`` writes (381-384)."""
        return (self.in_image.cpu().numpy(), self.in_fidelity.cpu().numpy(), self.in_noise.cpu().numpy(), self.in_mask.cpu().numpy().astype(np.uint8))
