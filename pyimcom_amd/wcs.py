"""World coordinate systems on the device: what the reference's ``PyIMCOM_WCS`` reduces a WCS to (src/pyimcom/wcsutil.py:419-634: a FITS
TAN-SIP header, or for gwcs input -- type ``"ASTROPY+"`` -- a fitted TAN-SIP plus a bilinear error map), and the functions that are made of
it: ``compareutils.map_sca2sca`` and ``get_overlap_matrix`` (src/pyimcom/utils/compareutils.py:63-178) and ``wcsutil.get_pix_area``
(wcsutil.py:688-788).  The binding (seam 16):

    w = pyimcom_amd.wcs.DeviceWCS.from_pyimcom(inwcs)          # or from_header(header), from_astropy(astropy_wcs)
    xf, yf, is_in_ref = pyimcom_amd.wcs.map_sca2sca(target_wcs, ref_wcs, pad=0)
    ov = pyimcom_amd.wcs.get_overlap_matrix(list_of_wcs, pad=0, subsamp=8)
    area = pyimcom_amd.wcs.pix_area(inwcs, [0, 4088, 0, 4088], pad=1, ovsamp=1)
    eng.set_pair(a, b, wcs=(all_wcs[a], all_wcs[b]))           # pyimcom_amd.destripe: the positions are formed on the device
                                                               # (keep_positions=False: inside the destripe kernels, nothing stored)

csrc/wcs.hip gives every point one owner thread; the descriptors travel as kernel arguments (csrc/wcs_core.h holds the arithmetic).

WHAT IS VERIFIED AND WHAT IS NOT.  astropy, gwcs and asdf are not installed where this code is built and tested.  The arithmetic is that of
the published definitions -- FITS WCS papers I and II (Greisen & Calabretta 2002; Calabretta & Greisen 2002) and the SIP convention (Shupe
et al. 2005) -- and the device is compared with those definitions evaluated in 40-digit arithmetic (tests/wcs_reference.py); the error map
is compared with scipy's ``RegularGridInterpolator``.  Agreement with astropy / wcslib has NOT been checked; tests/test_gpu_wcs.py holds
that comparison behind ``pytest.importorskip("astropy")``.  astropy's ``all_world2pix`` iterates to 1e-4 pixel and ignores AP / BP; the
inverse here is converged (Newton, steps below 2^-40 pixel), so the two may differ by astropy's tolerance.

Served: ``TAN`` / ``TAN-SIP`` (orders 0 .. 9, ``A_ORDER`` and ``B_ORDER`` independent) and ``STG``, two axes, CD or PC + CDELT or CDELT.
Refused (``ImcomError``, IMCOM_ERR_UNSUPPORTED): every other projection, ``PV`` terms, look-up distortions, ``CROTA``, more axes; a gwcs
model (``from_pyimcom`` of type ``"GWCS"``: TypeError -- it is arbitrary Python).

The error map: each point takes its own correction, table axes (y, x), which is what ``LocWCS.err_interp`` documents.  The reference's
``pos[::-1, :]`` (wcsutil.py:516, 589) reverses the order of the points instead of the two columns; that is not reproduced.

What stays on the host: FITS / ASDF, fitting the SIP and the error map of a gwcs, the cap algebra of ``getfootprint``.  (HEALPix: pyimcom_amd.healpix.)  A numpy
input gives numpy results; a tensor on a device gives tensors on that device, with no host round trip."""

import ctypes as C
from collections.abc import Mapping

import numpy as np

from ._dev import DEVICE, bound_context, is_torch, staged
from ._lib import MEM_DEVICE, ImcomError, check, lib, ptr

__all__ = ["DeviceWCS", "as_device_wcs", "error_table", "map_sca2sca", "get_overlap_matrix", "footprint_cap", "caps_can_touch", "overlap_count", "pix_area", "rotation_matrix", "sip_index",
           "DESC_LEN", "MAX_ORDER", "TAN", "STG"]

IMCOM_ERR_UNSUPPORTED = -4
TAN, STG = 0, 1
MAX_ORDER = 9
NCOEF = (MAX_ORDER + 1) * (MAX_ORDER + 2) // 2
(D_PROJ, D_CRPIX, D_CD, D_ROT, D_AORDER, D_BORDER, D_NITER, D_A) = (0, 1, 3, 7, 16, 17, 18, 20)
D_B = D_A + NCOEF
DESC_LEN = D_B + NCOEF  # 130 (csrc/wcs_core.h, include/imcom_hip.h)
SCA_NSIDE = 4088        # Settings.sca_nside, the default array_shape


def _unsupported(msg):
    return ImcomError(IMCOM_ERR_UNSUPPORTED, "wcs: " + msg)


def sip_index(p, q):
    """Where A_p_q sits in its block of the descriptor."""
    return p * (MAX_ORDER + 1) - p * (p - 1) // 2 + q


def rotation_matrix(crval1, crval2, lonpole):
    """R [3, 3] with native unit vector = R (celestial unit vector): Paper II eq. (2) for a zenithal projection (theta_0 = 90 deg), whose
    native pole is at (alpha_p, delta_p) = CRVAL, with phi_p = LONPOLE.  Formed in extended precision where numpy has it and rounded once."""
    ld = np.longdouble
    deg = ld(4) * np.arctan(ld(1)) / ld(180)
    a, d, p = ld(crval1) * deg, ld(crval2) * deg, ld(lonpole) * deg
    sa, ca, sd, cd, sp, cp = np.sin(a), np.cos(a), np.sin(d), np.cos(d), np.sin(p), np.cos(p)
    if float(crval2) == 90.0:
        sd, cd = ld(1), ld(0)
    if float(crval2) == -90.0:
        sd, cd = ld(-1), ld(0)
    R = [[-sa * sp - ca * cp * sd, ca * sp - sa * cp * sd, cp * cd],
         [sa * cp - ca * sp * sd, -ca * cp - sa * sp * sd, sp * cd],
         [ca * cd, sa * cd, sd]]
    return np.array([[float(v) for v in row] for row in R], dtype=np.float64)


def error_table(errmap, a=8, n_pad=None, use_float32=False):
    """The padded table of ``LocWCS.err_interp`` (wcsutil.py:388-403) from a raw ``errmap`` [2, N, N]: (table [2, N + 2, N + 2], lo, hi) with
    the end nodes at lo = -n_pad and hi = N + n_pad - 1 and the end values extrapolated linearly from the ``a`` pixels next to each edge
    (columns first, then rows, so that the corners come from the padded columns).  n_pad defaults to N // 2, PyIMCOM_WCS's choice."""
    errmap = np.asarray(errmap)
    if errmap.ndim != 3 or errmap.shape[0] != 2 or errmap.shape[1] != errmap.shape[2]:
        raise ValueError(f"wcs: an error map of shape {errmap.shape}, expected (2, N, N)")
    N = errmap.shape[1]
    n_pad = N // 2 if n_pad is None else n_pad
    if not (1 <= a <= N - 1) or n_pad <= 0:
        raise ValueError(f"wcs: a = {a}, n_pad = {n_pad} for an error map of {N} pixels a side")
    t = np.zeros((2, N + 2, N + 2), dtype=np.float32 if use_float32 else errmap.dtype)
    t[:, 1:-1, 1:-1] = errmap
    slope = n_pad / a
    for axis in (2, 1):  # the end columns first, then the end rows, so that the corners come from the padded columns
        v = np.moveaxis(t, axis, 0)  # (a view: node index first)
        v[0] = v[1] + slope * (v[1] - v[1 + a])
        v[-1] = v[-2] + slope * (v[-2] - v[-2 - a])
    return t, float(-n_pad), float(N + n_pad - 1)


def _projection(ctype1, ctype2):
    c1, c2 = str(ctype1).strip().upper(), str(ctype2).strip().upper()
    if not (c1.startswith("RA--") and c2.startswith("DEC-")):
        raise _unsupported(f"axes {c1!r}, {c2!r}: served is (RA, DEC) in this order")
    a1, a2 = c1[5:], c2[5:]
    if a1 != a2:
        raise _unsupported(f"axes {c1!r}, {c2!r} name different projections")
    if a1 in ("TAN", "TAN-SIP"):
        return TAN, a1.endswith("SIP")
    if a1 == "STG":
        return STG, False
    raise _unsupported(f"projection {a1!r}: served are TAN, TAN-SIP and STG")


def _pack(proj, crpix, crval, cd, lonpole, a_order, a, b_order, b, niter=0):
    """The descriptor.  a, b: [order + 1, order + 1] arrays indexed [p, q], or None."""
    d = np.zeros(DESC_LEN, dtype=np.float64)
    d[D_PROJ] = proj
    d[D_CRPIX:D_CRPIX + 2] = np.asarray(crpix, dtype=np.float64)
    d[D_CD:D_CD + 4] = np.asarray(cd, dtype=np.float64).reshape(4)
    crval = [float(crval[0]), float(crval[1])]
    if lonpole is None or not np.isfinite(lonpole):
        lonpole = 0.0 if crval[1] == 90.0 else 180.0
    d[D_ROT:D_ROT + 9] = rotation_matrix(crval[0], crval[1], float(lonpole)).reshape(9)
    for order, coef, at, slot in ((a_order, a, D_A, D_AORDER), (b_order, b, D_B, D_BORDER)):
        order = int(order or 0)
        if order < 0 or order > MAX_ORDER:
            raise _unsupported(f"a SIP order of {order}; served are 0 .. {MAX_ORDER}")
        if order and coef is not None:
            coef = np.asarray(coef, dtype=np.float64)
            for p in range(order + 1):
                for q in range(order + 1 - p):
                    if p < coef.shape[0] and q < coef.shape[1]:
                        d[at + sip_index(p, q)] = coef[p, q]
            if not np.any(d[at:at + NCOEF]):
                order = 0
        else:
            order = 0
        d[slot] = order
    d[D_NITER] = int(niter)
    if not np.all(np.isfinite(d)):
        raise ValueError("wcs: a descriptor entry is not finite")
    if d[D_CD] * d[D_CD + 3] - d[D_CD + 1] * d[D_CD + 2] == 0.0:
        raise ValueError("wcs: the CD matrix is singular")
    return d, crval, float(lonpole)


class DeviceWCS:
    """One WCS as the device evaluates it: ``descriptor`` (float64 [130]), the optional error table, ``array_shape`` and ``constructortype``
    as a ``PyIMCOM_WCS`` has them, and its two methods."""

    def __init__(self, descriptor, table=None, array_shape=(SCA_NSIDE, SCA_NSIDE), constructortype="FITSHEADER", crval=None, lonpole=None):
        self.descriptor = np.ascontiguousarray(descriptor, dtype=np.float64)
        if self.descriptor.shape != (DESC_LEN,):
            raise ValueError(f"wcs: a descriptor of shape {self.descriptor.shape}, expected ({DESC_LEN},)")
        self.array_shape = tuple(int(v) for v in array_shape)
        self.constructortype = constructortype
        self.type = "ASTROPY+" if table is not None else "ASTROPY"
        self.crval, self.lonpole = crval, lonpole
        self.table = None
        self._tab_dev = {}
        if table is not None:
            values, lo, hi = table
            if not is_torch(values):
                values = np.ascontiguousarray(values)
                if values.dtype not in (np.float32, np.float64):
                    values = values.astype(np.float64)
            if values.ndim != 3 or values.shape[0] != 2 or values.shape[1] != values.shape[2] or values.shape[1] < 4:
                raise ValueError(f"wcs: an error table of shape {tuple(values.shape)}, expected (2, N + 2, N + 2)")
            if not (lo < 0 and hi > values.shape[1] - 3):
                raise ValueError(f"wcs: end nodes {lo}, {hi} of an error table of {values.shape[1]} nodes an axis")
            self.table = (values, float(lo), float(hi))

    @property
    def niter(self):
        return int(self.descriptor[D_NITER])

    # ---- constructors (no astropy import) ----
    @classmethod
    def from_header(cls, header, array_shape=None, table=None, niter=0, constructortype="FITSHEADER"):
        """Any mapping with FITS keys (an astropy ``Header`` is one)."""
        h = {str(k).strip().upper(): header[k] for k in header.keys() if str(k).strip()}
        if int(h.get("WCSAXES", 2) or 2) > 2 or any(k in h for k in ("CTYPE3", "CRPIX3", "CRVAL3")):  # (NAXIS counts the data's axes, not the WCS's)
            raise _unsupported("more than two axes")
        for k in h:
            if k.startswith(("PV1_", "PV2_", "PS1_", "PS2_")):
                raise _unsupported(f"{k}: PV / PS terms are not served")
            if k.startswith(("CPDIS", "CQDIS", "DP1", "DP2", "DQ1", "DQ2", "D2IM", "CROTA")):
                raise _unsupported(f"{k}: look-up distortions and CROTA are not served")
        proj, _ = _projection(h["CTYPE1"], h["CTYPE2"])
        if any(k in h for k in ("CD1_1", "CD1_2", "CD2_1", "CD2_2")):
            cd = [float(h.get(k, 0.0)) for k in ("CD1_1", "CD1_2", "CD2_1", "CD2_2")]
        else:
            pc = [float(h.get(k, dflt)) for k, dflt in (("PC1_1", 1.0), ("PC1_2", 0.0), ("PC2_1", 0.0), ("PC2_2", 1.0))]
            cdelt = [float(h.get("CDELT1", 1.0)), float(h.get("CDELT2", 1.0))]
            cd = [cdelt[0] * pc[0], cdelt[0] * pc[1], cdelt[1] * pc[2], cdelt[1] * pc[3]]
        ab = []
        for L in "AB":
            order = int(h.get(f"{L}_ORDER", 0) or 0)  # (read whenever present, with or without the -SIP suffix, as astropy does)
            if not 0 <= order <= MAX_ORDER:
                raise _unsupported(f"{L}_ORDER = {order}; served are 0 .. {MAX_ORDER}")
            coef = np.zeros((order + 1, order + 1))
            for p in range(order + 1):
                for q in range(order + 1 - p):
                    coef[p, q] = float(h.get(f"{L}_{p}_{q}", 0.0))
            ab += [order, coef]
        d, crval, lonpole = _pack(proj, [float(h["CRPIX1"]), float(h["CRPIX2"])], [h["CRVAL1"], h["CRVAL2"]], cd, h.get("LONPOLE"), ab[0], ab[1], ab[2], ab[3],
                                  niter)
        if array_shape is None:
            array_shape = (SCA_NSIDE, SCA_NSIDE)
        return cls(d, table, array_shape, constructortype, crval, lonpole)

    @classmethod
    def from_astropy(cls, w, array_shape=None, table=None, niter=0, constructortype="ASTROPY"):
        """Duck-typed: ``w.wcs.crpix / crval / ctype / lonpole``, ``cd`` or ``pc`` and ``cdelt``, ``w.sip.a / b``."""
        ww = w.wcs
        if int(getattr(ww, "naxis", 2)) != 2:
            raise _unsupported("more than two axes")
        for name in ("cpdis1", "cpdis2", "det2im1", "det2im2"):
            if getattr(w, name, None) is not None:
                raise _unsupported(f"{name}: look-up distortions are not served")
        get_pv = getattr(ww, "get_pv", None)
        if get_pv is not None and len(get_pv()):
            raise _unsupported("PV terms are not served")
        proj, _ = _projection(ww.ctype[0], ww.ctype[1])
        try:
            cd = ww.cd
        except AttributeError:
            cd = None
        if cd is None:
            pc, cdelt = np.asarray(ww.pc, dtype=np.float64), np.asarray(ww.cdelt, dtype=np.float64)
            cd = [cdelt[0] * pc[0, 0], cdelt[0] * pc[0, 1], cdelt[1] * pc[1, 0], cdelt[1] * pc[1, 1]]
        sip = getattr(w, "sip", None)
        a = b = None
        ao = bo = 0
        if sip is not None:
            a, b = getattr(sip, "a", None), getattr(sip, "b", None)
            ao = int(getattr(sip, "a_order", 0 if a is None else np.shape(a)[0] - 1) or 0)
            bo = int(getattr(sip, "b_order", 0 if b is None else np.shape(b)[0] - 1) or 0)
        d, crval, lonpole = _pack(proj, ww.crpix, ww.crval, cd, getattr(ww, "lonpole", None), ao, a, bo, b, niter)
        if array_shape is None:
            array_shape = getattr(w, "array_shape", None) or (SCA_NSIDE, SCA_NSIDE)
        return cls(d, table, array_shape, constructortype, crval, lonpole)

    @classmethod
    def from_pyimcom(cls, w):
        """A ``PyIMCOM_WCS``: type "ASTROPY" -> its ``obj``; "ASTROPY+" -> ``obj``, the tables out of ``w.err[k].grid`` and ``.values``, and
        ``w.niter``; "GWCS" -> TypeError."""
        kind = getattr(w, "type", None)
        if kind == "GWCS":
            raise TypeError("wcs: a PyIMCOM_WCS of type 'GWCS' wraps a gwcs model, which is arbitrary Python; construct it without noconvert")
        shape = getattr(w, "array_shape", None) or (SCA_NSIDE, SCA_NSIDE)
        ctype = getattr(w, "constructortype", "ASTROPY")
        if kind == "ASTROPY":
            return cls.from_astropy(w.obj, shape, constructortype=ctype)
        if kind != "ASTROPY+":
            raise TypeError(f"wcs: a PyIMCOM_WCS of type {kind!r}")
        planes = []
        nodes = None
        for k in (0, 1):
            gy, gx = (np.asarray(g, dtype=np.float64) for g in w.err[k].grid)
            v = np.asarray(w.err[k].values)
            n2 = len(gx)
            if len(gy) != n2 or v.shape != (n2, n2) or not np.array_equal(gx, gy) or not np.array_equal(gx[1:-1], np.arange(n2 - 2)) or (
                    nodes is not None and not np.array_equal(nodes, gx)):
                raise _unsupported("an error interpolator whose grid is not err_interp's (nodes lo, 0, 1, .., N - 1, hi on both axes)")
            nodes = gx
            planes.append(v)
        dt = np.float32 if all(p.dtype == np.float32 for p in planes) else np.float64
        table = (np.stack([p.astype(dt, copy=False) for p in planes]), float(nodes[0]), float(nodes[-1]))
        return cls.from_astropy(w.obj, shape, table=table, niter=int(w.niter), constructortype=ctype)

    # ---- device ----
    def _table_args(self, dev):
        """(pointer, is float64, nodes an axis, lo, hi) of the error table on ``dev``; the tensor is kept."""
        if self.table is None:
            return None, 0, 0, 0.0, 0.0
        import torch

        values, lo, hi = self.table
        t = self._tab_dev.get(str(dev))
        if t is None:
            t = staged(values, dev)
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
            self._tab_dev[str(dev)] = t
        return ptr(t), int(t.dtype == torch.float64), int(t.shape[1]), lo, hi

    def _list(self, inverse, pos, origin, ctx=None, count_bad=False):
        """pos [n, 2] (numpy or tensor) -> [n, 2] of the same kind."""
        import torch

        origin = int(origin)
        if origin not in (0, 1):
            raise ValueError(f"wcs: origin {origin}")
        stay = is_torch(pos) and pos.is_cuda
        home = pos.device if is_torch(pos) else None  # (a tensor in gives a tensor out, on the device it came from)
        if len(pos.shape) != 2 or pos.shape[1] != 2:
            raise ValueError(f"wcs: positions of shape {tuple(pos.shape)}, expected (N, 2)")
        t = staged(pos, pos.device if stay else DEVICE, astype=np.float64)
        ctx = bound_context(t.device, ctx)
        out = torch.empty_like(t)
        nbad = C.c_long(0)
        tab = self._table_args(t.device)
        fn = lib.imcom_wcs_world2pix if inverse else lib.imcom_wcs_pix2world
        check(fn(ctx.handle, ptr(self.descriptor), tab[0], tab[1], tab[2], tab[3], tab[4], ptr(t), t.shape[0], origin, ptr(out),
                 C.byref(nbad) if count_bad else None, MEM_DEVICE))
        res = out if stay else (out.to(home) if home is not None else out.cpu().numpy())
        return (res, nbad.value) if count_bad else res

    def _call(self, inverse, args):
        """The 2-argument and 3-argument forms of wcsutil.py:524-560 / 598-634."""
        if len(args) == 2:
            pos = args[0]
            return self._list(inverse, pos if is_torch(pos) else np.array(pos, dtype=np.float64).reshape(-1, 2), args[1])
        if len(args) != 3:
            raise TypeError("wcs: (pos, origin) or (pos, pos2, origin)")
        a, b, origin = args
        if is_torch(a):
            import torch

            o = self._list(inverse, torch.stack((a.reshape(-1).to(torch.float64), b.reshape(-1).to(torch.float64).to(a.device)), dim=1), origin)
            return o[:, 0].reshape(a.shape), o[:, 1].reshape(b.shape)
        if isinstance(a, np.ndarray):
            o = self._list(inverse, np.vstack((a.ravel(), np.asarray(b).ravel())).T, origin)
            return o[:, 0].reshape(np.shape(a)), o[:, 1].reshape(np.shape(b))
        o = self._list(inverse, np.vstack((a, b)).T, origin)
        return o[0, 0], o[0, 1]

    def all_pix2world(self, *args):
        return self._call(0, args)

    def all_world2pix(self, *args):
        return self._call(1, args)


def as_device_wcs(w):
    """A DeviceWCS of a DeviceWCS (itself), a ``PyIMCOM_WCS``, an astropy-like WCS or a header-like mapping."""
    if isinstance(w, DeviceWCS):
        return w
    if hasattr(w, "constructortype") and hasattr(w, "type"):
        return DeviceWCS.from_pyimcom(w)
    if hasattr(w, "wcs"):
        return DeviceWCS.from_astropy(w)
    if isinstance(w, Mapping) or hasattr(w, "keys"):
        return DeviceWCS.from_header(w)
    raise TypeError(f"wcs: cannot make a DeviceWCS of {type(w).__name__}")


def _grid_axis(nside, pad, subsamp):
    """(lo, step, count) of compareutils.py:95-97: linspace(-pad, nside - 1 + pad, nside + 2 pad)[subsamp // 2 :: subsamp]."""
    full = int(nside) + 2 * int(pad)
    if subsamp > 1:
        return float(-pad + subsamp // 2), float(subsamp), len(range(subsamp // 2, full, subsamp))
    return float(-pad), 1.0, full


def _pix2pix(target, ref, grid=None, points=None, nside=SCA_NSIDE, pad=0, origin=0, want="xym", f32=False, device=DEVICE, ctx=None):
    """imcom_wcs_pix2pix: (x, y, mask, (count in ref, count NaN)); the outputs not in ``want`` are None."""
    import torch

    dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    if grid is not None:
        g = np.asarray(grid, dtype=np.float64)
        n, shape = int(g[2]) * int(g[5]), (int(g[5]), int(g[2]))
        pts = None
    else:
        pts = staged(points, dev, astype=np.float64)
        n, shape, g = pts.shape[0], (pts.shape[0],), None
    dt = torch.float32 if f32 else torch.float64
    x = torch.empty(shape, dtype=dt, device=dev) if "x" in want else None
    y = torch.empty(shape, dtype=dt, device=dev) if "x" in want else None
    m = torch.empty(shape, dtype=torch.uint8, device=dev) if "m" in want else None
    counts = np.zeros(2, dtype=np.int64)
    ta, tb = target._table_args(dev), ref._table_args(dev)
    check(lib.imcom_wcs_pix2pix(ctx.handle, ptr(target.descriptor), ta[0], ta[1], ta[2], ta[3], ta[4], ptr(ref.descriptor), tb[0], tb[1], tb[2], tb[3], tb[4],
                                ptr(pts), ptr(g), n, int(origin), float(nside), float(pad), ptr(x), ptr(y), int(f32), ptr(m), ptr(counts), MEM_DEVICE))
    return x, y, m, (int(counts[0]), int(counts[1]))


def map_sca2sca(target_wcs, ref_wcs, pad=0, dtype=np.float64, subsamp=1, device_out=False, device=DEVICE, ctx=None):
    """``compareutils.map_sca2sca`` (compareutils.py:63-106): (xf, yf, is_in_ref) of the target's pixel grid in the reference, through the
    unit vector alone.  dtype: np.float64 or np.float32 (the cast follows the mask, which is formed from the float64 positions).
    ``device_out``: tensors on ``device`` instead of numpy arrays."""
    target, ref = as_device_wcs(target_wcs), as_device_wcs(ref_wcs)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError(f"wcs: positions as {dtype}; served are float64 and float32")
    nside = target.array_shape[-1]
    lo, step, cnt = _grid_axis(nside, pad, int(subsamp))
    x, y, m, _ = _pix2pix(target, ref, grid=[lo, step, cnt, lo, step, cnt], nside=nside, pad=pad, f32=dtype == np.float32, device=device, ctx=ctx)
    m = m.to(bool)
    if device_out:
        return x, y, m
    return x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy()


def overlap_count(target_wcs, ref_wcs, pad=0, subsamp=1, device=DEVICE, ctx=None):
    """(points of the target's grid inside the reference, points of the grid): the count-only launch."""
    target, ref = as_device_wcs(target_wcs), as_device_wcs(ref_wcs)
    nside = target.array_shape[-1]
    lo, step, cnt = _grid_axis(nside, pad, int(subsamp))
    counts = _pix2pix(target, ref, grid=[lo, step, cnt, lo, step, cnt], nside=nside, pad=pad, want="", device=device, ctx=ctx)[3]
    return counts[0], cnt * cnt


_CORNER_SIGNS = np.array([[0.0, 0.0], [-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0]])  # the centre, then the four corners (x, y)


def _unit_vectors(ra, dec):
    """[n, 3] unit vectors of (ra, dec) in degrees."""
    a, d = np.deg2rad(ra), np.deg2rad(dec)
    return np.stack((np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)), axis=-1)


def footprint_cap(wcs, pad):
    """The spherical cap that holds an SCA padded by ``pad`` pixels a side (what compareutils.getfootprint, lines 23-60, describes):
    (unit vector of the chip's centre, 1 - cos of the largest angle from it to a padded corner).  The five sky positions come from the
    device's ``all_pix2world``; the cap algebra is numpy's."""
    nside = wcs.array_shape[-1]
    middle, reach = (nside - 1.0) / 2.0, nside / 2.0 + pad
    pix = middle + reach * _CORNER_SIGNS
    ra, dec = wcs.all_pix2world(pix[:, 0].copy(), pix[:, 1].copy(), 0)
    v = _unit_vectors(ra, dec)
    return v[0], float(np.max(1.0 - v[1:] @ v[0]))


def caps_can_touch(centres, p):
    """[N, N] bool: two caps can share a point when the angle between their centres is below the sum of their radii, i.e. (radii summing
    to less than pi) centre . centre > cos(theta_i + theta_j); p = 1 - cos(theta) (the test of compareutils.py:148-159, as the angle sum)."""
    c = 1.0 - np.asarray(p, dtype=np.float64)
    sn = np.sqrt(np.clip(1.0 - c * c, 0.0, None))
    return centres @ centres.T > np.outer(c, c) - np.outer(sn, sn)


def get_overlap_matrix(list_of_wcs, pad=0, verbose=False, subsamp=1, device=DEVICE, ctx=None):
    """``compareutils.get_overlap_matrix`` (compareutils.py:109-178): float32 [N, N], 1 on the diagonal, 0 for chips whose caps cannot touch,
    else the fraction of chip i's (sub-sampled, padded) pixel grid that lands inside chip j, for i > j, mirrored to [j, i].  One count-only
    launch a candidate pair; no position array is formed."""
    ws = [as_device_wcs(w) for w in list_of_wcs]
    caps = [footprint_cap(w, float(pad)) for w in ws]
    touch = caps_can_touch(np.array([c[0] for c in caps]).reshape(len(ws), 3), [c[1] for c in caps])
    ov = touch.astype(np.float32)
    if verbose:
        print(f"overlap matrix of {len(ws)} chips: {int(np.count_nonzero(np.tril(touch, -1)))} candidate pairs")
    for i, j in zip(*np.nonzero(np.tril(touch, -1))):
        inside, size = overlap_count(ws[i], ws[j], pad=pad, subsamp=subsamp, device=device, ctx=ctx)
        ov[i, j] = ov[j, i] = np.float32(inside / size)
        if verbose:
            print(f"  chip {i} in chip {j}: {ov[i, j]:.6f}", flush=True)
    return ov


def _area_axis(lo, hi, pad, ovsamp):
    """The centres of the ovsamp sub-pixels of the pixels lo - pad .. hi + pad - 1 (wcsutil.py:718-726), evenly spaced."""
    half = 0.5 / ovsamp
    return np.linspace(lo - 0.5 + half - pad, hi - 0.5 - half + pad, ovsamp * (hi - lo + 2 * pad))


def pix_area(wcs, region=(0, SCA_NSIDE, 0, SCA_NSIDE), pad=1, ovsamp=1, device_out=False, device=DEVICE, ctx=None, info=None):
    """``wcsutil.get_pix_area`` (wcsutil.py:688-788): the effective pixel areas in square degrees, shape (ovsamp (y1 - y0), ovsamp (x1 - x0)).
    It differences ra in degrees as the reference does, so its own noise is about ulp(ra) / (ra step).  ``info`` (a dict): receives
    "rotated", whether the footprint was turned away from the prime meridian (lines 740-749)."""
    import torch

    w = as_device_wcs(wcs)
    xmin, xmax, ymin, ymax = (int(v) for v in region)
    pad, ovsamp = int(pad), int(ovsamp)
    if pad < 1 or ovsamp < 1 or xmax <= xmin or ymax <= ymin:
        raise ValueError(f"wcs: region {list(region)}, pad {pad}, ovsamp {ovsamp}")
    xs, ys = _area_axis(xmin, xmax, pad, ovsamp), _area_axis(ymin, ymax, pad, ovsamp)
    dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    xs_d, ys_d = torch.as_tensor(xs).to(dev), torch.as_tensor(ys).to(dev)
    op = ovsamp * pad
    area = torch.empty((len(ys) - 2 * op, len(xs) - 2 * op), dtype=torch.float64, device=dev)
    tab = w._table_args(dev)
    rotated = C.c_int(0)
    check(lib.imcom_wcs_pix_area(ctx.handle, ptr(w.descriptor), tab[0], tab[1], tab[2], tab[3], tab[4], ptr(xs_d), len(xs), ptr(ys_d), len(ys), op, float(pad),
                                 ptr(area), C.byref(rotated), MEM_DEVICE))
    if info is not None:
        info["rotated"] = bool(rotated.value)
    return area if device_out else area.cpu().numpy()
