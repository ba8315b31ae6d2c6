"""The catalog of injected stars on the device: the per-star loop of ``StarsAnal.__call__`` (reference src/pyimcom/analysis.py:1000-1057,
driven by ``_BlkGrp.get_star_catalog`` 1309-1371) and of ``gen_starcube_nonoise`` (src/pyimcom/diagnostics/starcube_nonoise.py:186-237), and
the adaptive moments of a PSF (psfutil.py:516).  The binding (seam 15):

    moms = pyimcom_amd.starcat.adaptive_moments(image)                         # galsim.Image(image).FindAdaptiveMom(strict=False)
    sub_cat = pyimcom_amd.starcat.star_catalog(map_, x, y, forced_scale=..., fidelity=(codes, bels), inweight=..., n2=..., uc=..., ...)
    pos, image = pyimcom_amd.starcat.starcube_rows(map_, x, y, ibx, iby, force_scale=..., fidelity=(codes, bels), inweight=..., n2=...)
    fhist = pyimcom_amd.starcat.fidelity_histogram(codes, bels, bdpad)

csrc/starmom.hip takes one workgroup a star: the 79 x 79 cut goes into LDS once, the adaptive-moment iteration runs on it, then the fourth
moments and the forced-scale moments, all in float64 with sums reduced in a fixed order; a second kernel gives the means and ``np.std`` of
the 15 x 15 windows of the maps, a third the cuts themselves.

WHAT IS VERIFIED AND WHAT IS NOT.  GalSim is not installed where this code is built and tested.  The adaptive-moment iteration is restated
from the published algorithm (Bernstein & Jarvis 2002; Hirata & Seljak 2003) with GalSim's ``HSMParams`` defaults as the defaults of
``AdaptiveMomParams``; the device is compared with a float64 numpy restatement of the same iteration (tests/starcat_reference.py), with
analysis (a sampled elliptical Gaussian is its own fixed point) and, for everything but the ``FindAdaptiveMom`` call, with the reference's
own statements.  Agreement with an installed GalSim has NOT been checked; tests/test_starcat_host.py holds that comparison behind
``pytest.importorskip("galsim")``.

What stays on the host and with the caller: the WCS and HEALPix (``query_disc``, ``pix2ang``, ``all_world2pix``), FITS, ``np.savetxt`` and the
figures; the caller passes ``x, y``.  ``rint`` and the int16 casts of ``xi, yi``, the ``bdpad`` selection and ``wt[yi // n2, xi // n2]`` are
index work done here in numpy.  A numpy input gives numpy results; a tensor on a device is read in place and the results stay there."""

import ctypes as C

import numpy as np

from ._dev import DEVICE, bound_context, device_of, is_torch, np_dtype, staged, to_host, torch_dtype  # noqa: F401 (DEVICE: a public name here)
from ._lib import MEM_DEVICE, StarParams, check, lib, ptr
from . import reportstats

__all__ = ["AdaptiveMomParams", "AdaptiveMoments", "adaptive_moments", "star_moments", "star_catalog", "starcube_rows", "star_cuts", "window_stats",
           "fidelity_table", "fidelity_histogram", "cumulative", "select_stars", "COLUMNS", "STATUS_MESSAGES", "MAX_SIDE", "NCOL"]

MAX_SIDE = 127
# analysis.py:818-849 (ColDescr), in order
COLUMNS = ["RA", "DEC", "X_POS", "Y_POS", "AMPLITUDE", "OFFSET_X", "OFFSET_Y", "WIDTH", "SHAPE_G1", "SHAPE_G2", "M42_REAL", "M42_IMAG", "FORCED_PLUS",
           "FORCED_CROSS", "FIDELITY", "COVERAGE", "MEAN_UC", "MEAN_SIGMA", "STD_TSUM", "MEAN_NEFF"]
STATUS_MESSAGES = {0: "", 1: "Error: non positive definite adaptive moments!", 2: "Error: empty bounds in adaptive moments!",
                   3: "Error: adaptive moment or centroid shift too large!", 4: "Error: too many iterations in adaptive moments!",
                   5: "Error: NaN in adaptive moments!"}
# the columns of imcom_star_moments (csrc/starmom_core.h, SmCol)
(_AMP, _X, _Y, _SIGMA, _E1, _E2, _G1, _G2, _RHO4, _NITER, _STATUS, _CF, _SUM_WTI, _SUM_RE, _SUM_IM, _SUM_WTI2, _SUM_PLUS, _SUM_CROSS, _M42RE, _M42IM, _FPLUS,
 _FCROSS, NCOL) = range(23)


class AdaptiveMomParams:
    """The constants of the iteration; the defaults are GalSim's ``HSMParams`` defaults."""

    def __init__(self, convergence_threshold=1e-6, max_mom2_iter=400, bound_correct_wt=0.25, max_amoment=8000.0, max_ashift=15.0, max_moment_nsig2=25.0,
                 guess_sig=5.0):
        self.convergence_threshold, self.max_mom2_iter, self.bound_correct_wt = float(convergence_threshold), int(max_mom2_iter), float(bound_correct_wt)
        self.max_amoment, self.max_ashift, self.max_moment_nsig2, self.guess_sig = float(max_amoment), float(max_ashift), float(max_moment_nsig2), float(guess_sig)

    def _c(self):
        return StarParams(self.convergence_threshold, self.bound_correct_wt, self.max_amoment, self.max_ashift, self.max_moment_nsig2, self.guess_sig,
                          self.max_mom2_iter, 0)


def _frame(a, kinds):
    """(device tensor with unit column stride, was a tensor on a device)."""
    stay = is_torch(a) and a.is_cuda
    t = staged(a, device_of(a), layout="any")
    if np_dtype(t).name not in kinds or t.dim() != 2:
        raise TypeError(f"a 2-D array of {' / '.join(kinds)}, not {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, stay


def _ints(a, device, what):
    import torch

    a = np.ascontiguousarray(to_host(a))
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise TypeError(f"{what}: a 1-D integer array, not {a.dtype} {a.shape}")
    return torch.as_tensor(a.astype(np.int32)).to(device)


def _moments(t, ox, oy, w, h, forced_scale, params, ctx=None):
    """imcom_star_moments on the device tensor ``t``: float64 [nstar, NCOL] on the device."""
    import torch

    if w > MAX_SIDE or h > MAX_SIDE or w < 1 or h < 1:
        check(lib.imcom_star_sizes(0, int(w), int(h), 0, (C.c_long * 4)()))  # (raises IMCOM_ERR_UNSUPPORTED with the library's message)
    ctx = bound_context(t.device, ctx)
    ox, oy = _ints(ox, t.device, "ox"), _ints(oy, t.device, "oy")
    if ox.shape != oy.shape:
        raise ValueError("the stars' x and y differ in length")
    out = torch.zeros((ox.numel(), NCOL), dtype=torch.float64, device=t.device)
    par = (params or AdaptiveMomParams())._c()
    check(lib.imcom_star_moments(ctx.handle, ptr(t), int(t.dtype == torch.float64), t.shape[0], t.shape[1], t.stride(0), ptr(ox), ptr(oy), ox.numel(), int(w), int(h),
                                 C.cast(C.pointer(par), C.c_void_p), float(forced_scale), ptr(out), MEM_DEVICE))
    return out


class AdaptiveMoments:
    """What ``FindAdaptiveMom(strict=False)`` returns, for k images at once: arrays [k] (numpy, or tensors on the device if the images were)
    ``moments_amp``, ``moments_centroid_x`` / ``_y`` (GalSim's 1-based coordinates), ``moments_sigma``, ``e1``, ``e2``, ``g1``, ``g2``,
    ``moments_rho4``, ``moments_n_iter``, ``moments_status`` and the list ``error_message`` ("" for a star that converged).  Of a failed
    image only status, iterations and message mean anything (amp 0, sigma -1, rho4 -1, as GalSim leaves them).  ``table`` is the raw
    [k, NCOL] result."""

    def __init__(self, table, stay, single):
        import torch

        host = table.cpu().numpy()
        self.table = table if stay else host
        self.moments_status = host[:, _STATUS].astype(np.int32)
        self.moments_n_iter = host[:, _NITER].astype(np.int32)
        self.error_message = [STATUS_MESSAGES[int(s)] for s in self.moments_status]
        failed = self.moments_status != 0
        for name, col in (("moments_amp", _AMP), ("moments_centroid_x", _X), ("moments_centroid_y", _Y), ("moments_sigma", _SIGMA), ("e1", _E1), ("e2", _E2),
                          ("g1", _G1), ("g2", _G2), ("moments_rho4", _RHO4)):
            v = host[:, col].copy()
            if col in (_SIGMA, _RHO4):
                v[failed] = -1.0
            setattr(self, name, torch.as_tensor(v).to(table.device) if stay else v)
        self.single = single

    def __len__(self):
        return len(self.moments_status)


def adaptive_moments(images, params=None, ctx=None):
    """``galsim.Image(a).FindAdaptiveMom(strict=False)`` for ``images`` [k, h, w] or [h, w] (float32 / float64; sides up to 127, even sides too:
    the start centroid is ((1 + w) / 2, (1 + h) / 2))."""
    import torch

    stay = is_torch(images) and images.is_cuda
    a = images if is_torch(images) else np.asarray(images)
    single = len(a.shape) == 2
    shape = ((1,) if single else ()) + tuple(a.shape)
    kind = a.dtype if is_torch(a) else torch_dtype(a.dtype)
    if len(shape) != 3 or kind not in (torch.float32, torch.float64):
        raise TypeError(f"adaptive_moments: float32 / float64 images [k, h, w] or [h, w], not {kind} {shape}")
    k, h, w = shape
    if h < 1 or w < 1:
        raise ValueError(f"adaptive_moments: images of {h} x {w} pixels")
    t = staged(a, device_of(a))  # (after the checks: a refused input is not uploaded)
    t = t.reshape(k * h, w) if k else torch.zeros((1, w), dtype=t.dtype, device=t.device)
    out = _moments(t, np.zeros(k, dtype=np.int32), np.arange(k, dtype=np.int32) * h, w, h, 0.0, params, ctx)
    return AdaptiveMoments(out, stay, single)


def _positions(x, y):
    """analysis.py:982-983, 993-994: (x, y float64, xi, yi int16 as ints, dx, dy)."""
    x, y = np.asarray(to_host(x), dtype=np.float64), np.asarray(to_host(y), dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y are 1-D arrays of one length")
    xi = np.rint(x).astype(np.int16)
    yi = np.rint(y).astype(np.int16)
    return x, y, xi, yi, x - xi, y - yi


def select_stars(x, y, n, bdpad):
    """analysis.py:967-973: the indices of the stars whose pixel lies at least ``bdpad`` inside the n x n frame."""
    _, _, xi, yi, _, _ = _positions(x, y)
    return np.where(np.logical_and(np.logical_and(xi >= bdpad, xi < n - bdpad), np.logical_and(yi >= bdpad, yi < n - bdpad)))[0]


def star_moments(frame, x, y, bd=40, forced_scale=0.0, params=None, ctx=None):
    """Columns 10-19 of the catalog for the stars at (x, y) of ``frame`` (float32 / float64 [ny, nx]): a dict of arrays [nstar] AMPLITUDE,
    OFFSET_X, OFFSET_Y, WIDTH, SHAPE_G1, SHAPE_G2, M42_REAL, M42_IMAG, FORCED_PLUS, FORCED_CROSS (zero for a star that failed, as the
    reference's ``continue`` leaves them), ``status``, ``n_iter`` and ``table`` (the raw [nstar, NCOL] result).  The cut of a star is
    frame[yi + 1 - bd : yi + bd, xi + 1 - bd : xi + bd], zero outside the frame."""
    import torch

    t, stay = _frame(frame, ("float32", "float64"))
    x, y, xi, yi, dx, dy = _positions(x, y)
    side = 2 * int(bd) - 1
    tab = _moments(t, xi.astype(np.int32) + 1 - int(bd), yi.astype(np.int32) + 1 - int(bd), side, side, forced_scale, params, ctx)
    ok = tab[:, _STATUS] == 0
    z = torch.zeros_like(tab[:, 0])
    dxt, dyt = torch.as_tensor(dx).to(t.device), torch.as_tensor(dy).to(t.device)
    cols = {"AMPLITUDE": tab[:, _AMP], "OFFSET_X": tab[:, _X] - bd - dxt, "OFFSET_Y": tab[:, _Y] - bd - dyt, "WIDTH": tab[:, _SIGMA], "SHAPE_G1": tab[:, _G1],
            "SHAPE_G2": tab[:, _G2], "M42_REAL": tab[:, _M42RE], "M42_IMAG": tab[:, _M42IM], "FORCED_PLUS": tab[:, _FPLUS], "FORCED_CROSS": tab[:, _FCROSS]}
    out = {k: torch.where(ok, v, z) for k, v in cols.items()}
    out["status"], out["n_iter"], out["table"] = tab[:, _STATUS].to(torch.int32), tab[:, _NITER].to(torch.int32), tab
    return out if stay else {k: v.cpu().numpy() for k, v in out.items()}


def fidelity_table(dtype, bels):
    """int16 [65536]: analysis.py:938-941 (the reference's own expression) on every code of a (u)int16 FIDELITY map, by bit pattern."""
    codes = reportstats._all_codes(dtype)
    with np.errstate(all="ignore"):
        fmap = codes.astype(np.float32) * bels / (-0.1)
        return np.floor(fmap).astype(np.int16)


def window_stats(map_, xi, yi, bd2=8, table=None, ctx=None):
    """(mean, np.std) [nstar] of map_[yi + 1 - bd2 : yi + bd2, xi + 1 - bd2 : xi + bd2], accumulated in float64 (two passes for the
    deviation).  ``map_``: float32 / float64, or int16 / uint16 codes with ``table`` (int16 [65536]): the window is then of table[code],
    summed as integers.  Slices as numpy slices them; NaN for an empty window."""
    import torch

    coded = table is not None
    t, stay = _frame(map_, ("int16", "uint16") if coded else ("float32", "float64"))
    ctx = bound_context(t.device, ctx)
    xi, yi = _ints(xi, t.device, "xi"), _ints(yi, t.device, "yi")
    tab = staged(np.asarray(table, dtype=np.int16), t.device) if coded else None
    if coded and tab.numel() != 65536:
        raise ValueError("window_stats: a table of 65536 int16 values")
    out = torch.zeros((xi.numel(), 2), dtype=torch.float64, device=t.device)
    kind = 2 if coded else int(t.dtype == torch.float64)
    check(lib.imcom_star_window_stats(ctx.handle, ptr(t), kind, t.shape[0], t.shape[1], t.stride(0), ptr(tab), ptr(xi), ptr(yi), xi.numel(), int(bd2), ptr(out),
                                      MEM_DEVICE))
    return (out[:, 0], out[:, 1]) if stay else (out[:, 0].cpu().numpy(), out[:, 1].cpu().numpy())


def star_cuts(frame, xi, yi, bd=40, ctx=None):
    """float32 [nstar, 2 bd - 1, 2 bd - 1]: the cuts, ``np.pad(frame, bd)[yi + 1 : yi + 2 bd, xi + 1 : xi + 2 bd]`` (starcube_nonoise.py:190-196)."""
    import torch

    t, stay = _frame(frame, ("float32", "float64"))
    side = 2 * int(bd) - 1
    if side > MAX_SIDE or side < 1:
        check(lib.imcom_star_sizes(0, side, side, 0, (C.c_long * 4)()))
    ctx = bound_context(t.device, ctx)
    ox, oy = _ints(np.asarray(xi).astype(np.int64) + 1 - int(bd), t.device, "xi"), _ints(np.asarray(yi).astype(np.int64) + 1 - int(bd), t.device, "yi")
    out = torch.zeros((ox.numel(), side, side), dtype=torch.float32, device=t.device)
    check(lib.imcom_star_cuts(ctx.handle, ptr(t), int(t.dtype == torch.float64), t.shape[0], t.shape[1], t.stride(0), ptr(ox), ptr(oy), ox.numel(), side, side, ptr(out),
                              MEM_DEVICE))
    return out if stay else out.cpu().numpy()


def _coverage(inweight, n2, xi, yi):
    """analysis.py:937, 1049."""
    wt = np.sum(np.where(to_host(inweight) > 0.01, 1, 0), axis=0)
    return wt[yi // n2, xi // n2]


def star_catalog(frame, x, y, *, bd=40, bd2=8, forced_scale, fidelity, inweight=None, n2=None, uc=None, sigma=None, tsum=None, neff=None, empirical=False,
                 ra=None, dec=None, params=None, ctx=None):
    """``sub_cat`` float64 [npix, 20] of StarsAnal.__call__ (981-1057; columns ``COLUMNS``) for the stars at (x, y) -- already selected, 967-978:
    ``select_stars``.  ``fidelity`` = (codes int16 / uint16 [ny, nx], bels): the FIDELITY HDU as stored and ``HDU_to_bels`` of it; ``inweight``
    [nin, ny // n2, nx // n2] the INWEIGHT HDU; ``uc``, ``sigma``, ``tsum``, ``neff``: the float maps of ``get_output_map`` or None (the
    column is then -1); ``empirical``: STD_TSUM is 0 (1055-1056).  A star whose iteration fails keeps zeros from AMPLITUDE on (1005-1006)."""
    import torch

    x, y, xi, yi, _, _ = _positions(x, y)
    npix = len(x)
    cat = np.zeros((npix, len(COLUMNS)))
    col = {n: i for i, n in enumerate(COLUMNS)}
    cat[:, col["RA"]] = 0.0 if ra is None else to_host(ra)
    cat[:, col["DEC"]] = 0.0 if dec is None else to_host(dec)
    cat[:, col["X_POS"]], cat[:, col["Y_POS"]] = x, y
    if npix == 0:
        return cat
    m = star_moments(frame, x, y, bd, forced_scale, params, ctx)
    status = to_host(m["status"])
    ok = status == 0
    for name in COLUMNS[4:14]:
        cat[:, col[name]] = to_host(m[name])
    codes, bels = fidelity
    rows = np.zeros((npix, 6))
    rows[:, 0] = to_host(window_stats(codes, xi, yi, bd2, table=fidelity_table(np_dtype(codes), bels), ctx=ctx)[0])
    rows[:, 1] = _coverage(inweight, int(n2), xi, yi)
    for j, (mp, which) in enumerate(((uc, 0), (sigma, 0), (tsum, 1), (neff, 0))):
        rows[:, 2 + j] = -1 if mp is None else to_host(window_stats(mp, xi, yi, bd2, ctx=ctx)[which])
    if empirical:
        rows[:, 4] = 0
    cat[ok, col["FIDELITY"]:] = rows[ok]
    if is_torch(frame) and frame.is_cuda:
        return torch.as_tensor(cat).to(frame.device)
    return cat


def starcube_rows(frame, x, y, ibx=0, iby=0, *, bd=40, bd2=8, force_scale, fidelity, inweight, n2, ra=None, dec=None, params=None, ctx=None):
    """(``newpos`` float64 [npix, 22], ``newimage`` float32 [npix, 2 bd - 1, 2 bd - 1]) of gen_starcube_nonoise (169-237) for one block:
    columns ra, dec, ibx, iby, x, y, xi, yi, dx, dy, then 10-19 as in the catalog, the fidelity mean and the coverage."""
    x, y, xi, yi, dx, dy = _positions(x, y)
    npix = len(x)
    pos = np.zeros((npix, 22))
    pos[:, 0], pos[:, 1] = 0.0 if ra is None else to_host(ra), 0.0 if dec is None else to_host(dec)
    pos[:, 2], pos[:, 3], pos[:, 4], pos[:, 5], pos[:, 6], pos[:, 7], pos[:, 8], pos[:, 9] = ibx, iby, x, y, xi, yi, dx, dy
    cube = to_host(star_cuts(frame, xi, yi, bd, ctx))
    if npix == 0:
        return pos, cube
    m = star_moments(frame, x, y, bd, force_scale, params, ctx)
    ok = to_host(m["status"]) == 0
    for j, name in enumerate(COLUMNS[4:14]):
        pos[:, 10 + j] = to_host(m[name])
    codes, bels = fidelity
    tail = np.zeros((npix, 2))
    tail[:, 0] = to_host(window_stats(codes, xi, yi, bd2, table=fidelity_table(np_dtype(codes), bels), ctx=ctx)[0])
    tail[:, 1] = _coverage(inweight, int(n2), xi, yi)
    pos[ok, 20:] = tail[ok]
    return pos, cube


def fidelity_histogram(codes, bels, bdpad, ctx=None):
    """uint32-valued int64 [81]: starcube_nonoise.py:142-143, the counts of floor(fidelity in dB) = 0 .. 80 inside the padding, through
    ``reportstats.coded_map_histogram`` (no kernel of its own)."""
    fmap = fidelity_table(np_dtype(codes), bels)
    table = np.where((fmap >= 0) & (fmap <= 80), fmap, 255).astype(np.uint8)
    bdpad = int(bdpad)
    n0, n1 = codes.shape
    return reportstats.coded_map_histogram(codes[bdpad:n0 - bdpad, bdpad:n1 - bdpad], table, 81, ctx=ctx)[:81]


def cumulative(fhist):
    """The two columns of ``_fidHist.txt`` (259-261): the share of each bin and the cumulative share."""
    fhist = np.asarray(fhist)
    return np.stack([fhist / np.sum(fhist), np.cumsum(fhist) / np.sum(fhist)], axis=1)
