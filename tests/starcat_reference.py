"""Float64 numpy restatement of the star catalog (reference src/pyimcom/analysis.py:1000-1057, StarsAnal.__call__, and
src/pyimcom/diagnostics/starcube_nonoise.py:186-237).  It imports nothing from the reference.

``find_adaptive_mom`` restates the adaptive-moment iteration that ``galsim.Image(a).FindAdaptiveMom(strict=False)`` runs -- the published
algorithm (Bernstein & Jarvis 2002; Hirata & Seljak 2003) with GalSim's ``HSMParams`` defaults as the defaults of ``Params``.  GalSim is not
installed where the fixtures are made, so THIS function is what tests/golden/starcat.npz records and what the device is compared with; its
agreement with an installed GalSim is checked by tests/test_starcat_host.py wherever GalSim exists, and nowhere else.

Pixel (column i, row j) of an h x w array has the coordinates (i + 1, j + 1), as ``galsim.Image(ndarray)`` has them.  The arithmetic that
decides which pixels are summed (the rows and the column range of each row) is written one operation a statement in the order of
csrc/starmom_core.h; numpy's float64 scalars round each once."""

import math
from types import SimpleNamespace

import numpy as np

STATUS_OK, STATUS_NOT_PD, STATUS_EMPTY, STATUS_TOO_LARGE, STATUS_TOO_MANY, STATUS_NAN = 0, 1, 2, 3, 4, 5
MESSAGES = {0: "", 1: "Error: non positive definite adaptive moments!", 2: "Error: empty bounds in adaptive moments!",
            3: "Error: adaptive moment or centroid shift too large!", 4: "Error: too many iterations in adaptive moments!",
            5: "Error: NaN in adaptive moments!"}

COLUMNS = ["RA", "DEC", "X_POS", "Y_POS", "AMPLITUDE", "OFFSET_X", "OFFSET_Y", "WIDTH", "SHAPE_G1", "SHAPE_G2", "M42_REAL", "M42_IMAG", "FORCED_PLUS",
           "FORCED_CROSS", "FIDELITY", "COVERAGE", "MEAN_UC", "MEAN_SIGMA", "STD_TSUM", "MEAN_NEFF"]  # analysis.py:818-849


class Params:
    def __init__(self, convergence_threshold=1e-6, max_mom2_iter=400, bound_correct_wt=0.25, max_amoment=8000.0, max_ashift=15.0, max_moment_nsig2=25.0,
                 guess_sig=5.0):
        self.convergence_threshold, self.max_mom2_iter, self.bound_correct_wt = float(convergence_threshold), int(max_mom2_iter), float(bound_correct_wt)
        self.max_amoment, self.max_ashift, self.max_moment_nsig2, self.guess_sig = float(max_amoment), float(max_ashift), float(max_moment_nsig2), float(guess_sig)


def _max(a, b):
    """std::max: the first argument unless it compares below the second (a NaN in front stays)."""
    return b if a < b else a


def _clip(v, bound):
    if v > bound:
        v = bound
    if v < -bound:
        v = -bound
    return v


def _div(a, b):
    """IEEE division of two floats (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def ellipse_ranges(x0, y0, Mxx, Mxy, Myy, h, w, nsig2):
    """The head of an iteration.  Returns (status, detM, Minv_xx, TwoMinv_xy, Minv_yy, iy, ix1, ix2, ends): the 1-based rows iy (int array)
    that hold pixels of the ellipse with their inclusive column ranges, and ``ends`` = the unrounded (x1, x2) of those rows with y0 -+ y2."""
    none = np.zeros(0, dtype=np.int64)
    detM = Mxx * Myy - Mxy * Mxy
    if not (detM > 0.0 and Mxx > 0.0 and Myy > 0.0):
        return STATUS_NOT_PD, detM, 0.0, 0.0, 0.0, none, none, none, None
    Minv_xx = Myy / detM
    TwoMinv_xy = (-2.0 * Mxy) / detM
    Minv_yy = Mxx / detM
    y2 = math.sqrt(nsig2 * Myy)
    lo, hi = _max(math.ceil(y0 - y2), 1.0), min(math.floor(y0 + y2), float(h))
    if not lo <= hi:
        return STATUS_EMPTY, detM, Minv_xx, TwoMinv_xy, Minv_yy, none, none, none, None
    iy = np.arange(int(lo), int(hi) + 1)
    dy = iy.astype(np.float64) - y0
    b = TwoMinv_xy * dy
    q = Minv_yy * dy
    qq = q * dy
    c = qq - nsig2
    bb = b * b
    a4 = 4.0 * Minv_xx
    a4c = a4 * c
    d = bb - a4c
    ok = d >= 0.0
    sqrtd = np.sqrt(np.where(ok, d, 0.0))
    inv2 = 0.5 / Minv_xx
    t1 = -b - sqrtd
    t2 = -b + sqrtd
    p1 = inv2 * t1
    p2 = inv2 * t2
    x1 = x0 + p1
    x2 = x0 + p2
    lo_x, hi_x = np.maximum(np.ceil(x1), 1.0), np.minimum(np.floor(x2), float(w))
    ok &= lo_x <= hi_x
    ends = (x1[ok], x2[ok], y0 - y2, y0 + y2)
    return -1, detM, Minv_xx, TwoMinv_xy, Minv_yy, iy[ok], lo_x[ok].astype(np.int64), hi_x[ok].astype(np.int64), ends


def weighted_sums(image, x0, y0, Minv_xx, TwoMinv_xy, Minv_yy, iy, ix1, ix2, reverse=False):
    """The seven sums A, Bx, By, Cxx, Cxy, Cyy, rho4 over the pixels of the ranges (and the sums of the terms' magnitudes)."""
    h, w = image.shape
    cols = np.arange(1, w + 1)
    sel = (cols[None, :] >= ix1[:, None]) & (cols[None, :] <= ix2[:, None])
    rr, cc = np.nonzero(sel)
    data = image[iy[rr] - 1, cc].astype(np.float64)
    dy = iy[rr].astype(np.float64) - y0
    dx = cols[cc].astype(np.float64) - x0
    b = TwoMinv_xy * dy
    rho2 = ((Minv_yy * dy) * dy + b * dx) + (Minv_xx * dx) * dx
    inten = np.exp(-0.5 * rho2) * data
    ix_, iy_ = inten * dx, inten * dy
    terms = np.stack([inten, ix_, iy_, ix_ * dx, ix_ * dy, iy_ * dy, (inten * rho2) * rho2])
    if reverse:
        terms = np.ascontiguousarray(terms[:, ::-1])
    return terms.sum(axis=1)


def step(state, sums, p):
    """The tail of an iteration (csrc/starmom_core.h, sm_step): ``state`` = dict of x0, y0, Mxx, Mxy, Myy, x00, y00, shiftscale0, iter.
    Returns (status, cf): status -1 while the iteration goes on."""
    s = state
    A, Bx, By, Cxx, Cxy, Cyy = (float(v) for v in sums[:6])
    two_psi = math.atan2(2.0 * s["Mxy"], s["Mxx"] - s["Myy"])
    tr = s["Mxx"] + s["Myy"]
    semi_a2 = 0.5 * (tr + (s["Mxx"] - s["Myy"]) * math.cos(two_psi)) + s["Mxy"] * math.sin(two_psi)
    semi_b2 = tr - semi_a2
    if not semi_b2 > 0.0:
        return STATUS_NOT_PD, s.get("cf", 1.0)
    shiftscale = math.sqrt(semi_b2)
    if s["iter"] == 0:
        s["shiftscale0"] = shiftscale
    dx = _div(2.0 * Bx, A * shiftscale)
    dy = _div(2.0 * By, A * shiftscale)
    dxx = 4.0 * (_div(Cxx, A) - 0.5 * s["Mxx"]) / semi_b2
    dxy = 4.0 * (_div(Cxy, A) - 0.5 * s["Mxy"]) / semi_b2
    dyy = 4.0 * (_div(Cyy, A) - 0.5 * s["Myy"]) / semi_b2
    bound = p.bound_correct_wt
    dx, dy, dxx, dxy, dyy = _clip(dx, bound), _clip(dy, bound), _clip(dxx, bound), _clip(dxy, bound), _clip(dyy, bound)
    cf = _max(abs(dx), abs(dy))
    cf = cf * cf
    cf = _max(cf, abs(dxx))
    cf = _max(cf, abs(dxy))
    cf = _max(cf, abs(dyy))
    cf = math.sqrt(cf) if cf == cf else cf
    if shiftscale < s["shiftscale0"]:
        cf *= s["shiftscale0"] / shiftscale
    s["x0"] += dx * shiftscale
    s["y0"] += dy * shiftscale
    s["Mxx"] += dxx * semi_b2
    s["Mxy"] += dxy * semi_b2
    s["Myy"] += dyy * semi_b2
    s["cf"] = cf
    s["iter"] += 1
    if (abs(s["Mxx"]) > p.max_amoment or abs(s["Mxy"]) > p.max_amoment or abs(s["Myy"]) > p.max_amoment or abs(s["x0"] - s["x00"]) > p.max_ashift
            or abs(s["y0"] - s["y00"]) > p.max_ashift):
        return STATUS_TOO_LARGE, cf
    if s["iter"] > p.max_mom2_iter:
        return STATUS_TOO_MANY, cf
    if cf != cf or A != A:
        return STATUS_NAN, cf
    if not cf > p.convergence_threshold:
        return STATUS_OK, cf
    return -1, cf


def find_adaptive_mom(image, params=None, reverse=False, trace=None):
    """The stand-in for ``galsim.Image(image).FindAdaptiveMom(strict=False)``: an object with ``error_message``, ``moments_status``,
    ``moments_amp``, ``moments_centroid`` (.x, .y), ``moments_sigma``, ``observed_shape`` (.e1, .e2, .g1, .g2), ``moments_rho4``,
    ``moments_n_iter`` and ``last_cf``.  ``reverse``: the sums are taken over the pixels in reversed order.  ``trace``: a list that receives, per
    iteration, (state before, rows, ix1, ix2, ends, sums, state after, status, cf)."""
    p = params or Params()
    image = np.asarray(image)
    h, w = image.shape
    s = {"x0": (1.0 + w) / 2.0, "y0": (1.0 + h) / 2.0, "Mxx": p.guess_sig * p.guess_sig, "Mxy": 0.0, "Myy": p.guess_sig * p.guess_sig, "shiftscale0": 0.0, "iter": 0,
         "cf": 1.0}
    s["x00"], s["y00"] = s["x0"], s["y0"]
    status, sums = -1, np.zeros(7)
    for _ in range(p.max_mom2_iter + 1):
        before = dict(s)
        status, detM, Minv_xx, TwoMinv_xy, Minv_yy, iy, ix1, ix2, ends = ellipse_ranges(s["x0"], s["y0"], s["Mxx"], s["Mxy"], s["Myy"], h, w, p.max_moment_nsig2)
        if status >= 0:
            break
        sums = weighted_sums(image, s["x0"], s["y0"], Minv_xx, TwoMinv_xy, Minv_yy, iy, ix1, ix2, reverse)
        status, cf = step(s, sums, p)
        if trace is not None:
            trace.append((before, iy, ix1, ix2, ends, sums, dict(s), status, cf))
        if status >= 0:
            break
    if status < 0:
        status = STATUS_TOO_MANY
    out = SimpleNamespace(moments_status=status, error_message=MESSAGES[status], moments_n_iter=s["iter"], last_cf=s["cf"], moments_amp=0.0,
                          moments_centroid=SimpleNamespace(x=0.0, y=0.0), moments_sigma=-1.0, observed_shape=SimpleNamespace(e1=0.0, e2=0.0, g1=0.0, g2=0.0),
                          moments_rho4=-1.0)
    if status != STATUS_OK:
        return out
    A = float(sums[0])
    out.moments_amp = 2.0 * A
    out.moments_centroid = SimpleNamespace(x=s["x0"], y=s["y0"])
    det = s["Mxx"] * s["Myy"] - s["Mxy"] * s["Mxy"]
    out.moments_sigma = math.sqrt(math.sqrt(det))
    tr = s["Mxx"] + s["Myy"]
    e1, e2 = (s["Mxx"] - s["Myy"]) / tr, 2.0 * s["Mxy"] / tr
    g = 1.0 / (1.0 + math.sqrt(1.0 - (e1 * e1 + e2 * e2)))
    out.observed_shape = SimpleNamespace(e1=e1, e2=e2, g1=e1 * g, g2=e2 * g)
    out.moments_rho4 = float(sums[6]) / A
    return out


def cut(frame, xi, yi, bd):
    """The cut of side 2 bd - 1 round (xi, yi), zero outside the frame: starcube_nonoise.py:190-196 (the slice where it fits, np.pad otherwise)."""
    xi, yi = int(xi), int(yi)
    return np.pad(frame, bd)[yi + 1:yi + 2 * bd, xi + 1:xi + 2 * bd]


def higher_moments(newimage, moms, forced_scale):
    """analysis.py:1016-1041 on one cut: (M42_REAL, M42_IMAG, FORCED_PLUS, FORCED_CROSS), the six sums, and the scale of each of the four
    columns, sum |terms| / |sum of the weights|."""
    h, w = newimage.shape
    newimage = newimage.astype(np.float64)
    x_, y_ = np.meshgrid(np.arange(1, w + 1) - moms.moments_centroid.x, np.arange(1, h + 1) - moms.moments_centroid.y)
    e1, e2 = moms.observed_shape.e1, moms.observed_shape.e2
    Mxx = moms.moments_sigma**2 * (1 + e1) / np.sqrt(1 - e1**2 - e2**2)
    Myy = moms.moments_sigma**2 * (1 - e1) / np.sqrt(1 - e1**2 - e2**2)
    Mxy = moms.moments_sigma**2 * e2 / np.sqrt(1 - e1**2 - e2**2)
    D = Mxx * Myy - Mxy**2
    zeta = D * (Mxx + Myy + 2 * np.sqrt(D))
    u_ = ((Myy + np.sqrt(D)) * x_ - Mxy * y_) / zeta**0.5
    v_ = ((Mxx + np.sqrt(D)) * y_ - Mxy * x_) / zeta**0.5
    wti = newimage * np.exp(-0.5 * (u_**2 + v_**2))
    t_re, t_im = wti * (u_**4 - v_**4), wti * (u_**3 * v_ + u_ * v_**3)
    wti2 = newimage * np.exp(-0.5 * (x_**2 + y_**2) / forced_scale**2)
    t_pl, t_cr = wti2 * (x_**2 - y_**2), wti2 * (2 * x_ * y_)
    sums = np.array([np.sum(wti), np.sum(t_re), np.sum(t_im), np.sum(wti2), np.sum(t_pl), np.sum(t_cr)])
    cols = np.array([sums[1] / sums[0], 2 * sums[2] / sums[0], sums[4] / sums[3] / forced_scale**2, sums[5] / sums[3] / forced_scale**2])
    scales = np.array([np.sum(np.abs(t_re)) / abs(sums[0]), 2 * np.sum(np.abs(t_im)) / abs(sums[0]), np.sum(np.abs(t_pl)) / abs(sums[3]) / forced_scale**2,
                       np.sum(np.abs(t_cr)) / abs(sums[3]) / forced_scale**2])
    return cols, sums, scales


def fidelity_map(codes, bels):
    """analysis.py:938-941."""
    fmap = codes.astype(np.float32) * bels / (-0.1)
    return np.floor(fmap).astype(np.int16)


def catalog(frame, x, y, bd, bd2, forced_scale, fidelity, inweight, n2, uc=None, sigma=None, tsum=None, neff=None, empirical=False, ra=None, dec=None,
            params=None):
    """The [npix, 20] table of StarsAnal.__call__ (981-1057) for stars at (x, y) whose cuts lie inside the frame or not (zero padding)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    npix = len(x)
    cat = np.zeros((npix, len(COLUMNS)))
    col = {n: i for i, n in enumerate(COLUMNS)}
    xi, yi = np.rint(x).astype(np.int16), np.rint(y).astype(np.int16)
    cat[:, col["RA"]] = 0.0 if ra is None else ra
    cat[:, col["DEC"]] = 0.0 if dec is None else dec
    cat[:, col["X_POS"]], cat[:, col["Y_POS"]] = x, y
    dx, dy = x - xi, y - yi
    wt = np.sum(np.where(inweight > 0.01, 1, 0), axis=0)
    fmap = fidelity_map(*fidelity)
    for k in range(npix):
        newimage = cut(frame, xi[k], yi[k], bd)
        moms = find_adaptive_mom(newimage, params)
        if moms.error_message != "":
            continue
        cat[k, col["AMPLITUDE"]] = moms.moments_amp
        cat[k, col["OFFSET_X"]] = moms.moments_centroid.x - bd - dx[k]
        cat[k, col["OFFSET_Y"]] = moms.moments_centroid.y - bd - dy[k]
        cat[k, col["WIDTH"]] = moms.moments_sigma
        cat[k, col["SHAPE_G1"]], cat[k, col["SHAPE_G2"]] = moms.observed_shape.g1, moms.observed_shape.g2
        cat[k, col["M42_REAL"]:col["FORCED_CROSS"] + 1] = higher_moments(newimage, moms, forced_scale)[0]
        central = np.s_[int(yi[k]) + 1 - bd2:int(yi[k]) + bd2, int(xi[k]) + 1 - bd2:int(xi[k]) + bd2]
        cat[k, col["FIDELITY"]] = np.mean(fmap[central])
        cat[k, col["COVERAGE"]] = wt[yi[k] // n2, xi[k] // n2]
        cat[k, col["MEAN_UC"]] = np.mean(uc[central]) if uc is not None else -1
        cat[k, col["MEAN_SIGMA"]] = np.mean(sigma[central]) if sigma is not None else -1
        cat[k, col["STD_TSUM"]] = np.std(tsum[central]) if tsum is not None else -1
        if empirical:
            cat[k, col["STD_TSUM"]] = 0
        cat[k, col["MEAN_NEFF"]] = np.mean(neff[central]) if neff is not None else -1
    return cat


# ---- the fixture of tests/golden/starcat.npz ----
N, BDS, BD2, N2, FORCED_SCALE, BELS = 96, (4, 8, 40), 8, 12, 0.40 / 0.11 * 0.7, 0.0002
# (nominal x, nominal y, flux, sigma, e1, e2, wing fraction); a star of OFFSETS is drawn that far from the nominal position the catalog is told
STARS = [
    (42.0, 14.0, 3.0, 2.5, 0.0, 0.0, 0.0),       # 0 round, centred on a pixel
    (14.3, 14.2, 2.0, 2.2, 0.2, 0.0, 0.0),       # 1 elliptical
    (14.49, 42.51, 4.0, 2.8, 0.1, -0.15, 0.0),   # 2 rotated, -+0.49 off the pixel
    (14.0, 70.0, 5.0, 2.4, 0.05, 0.08, 0.3),     # 3 power-law wings
    (42.0, 70.0, -2.5, 2.6, 0.0, 0.1, 0.0),      # 4 negative
    (82.0, 14.0, 3.0, 2.3, -0.1, 0.0, 0.0),      # 5 drawn 12 px from its nominal position: converges at bd = 40
    (90.0, 42.0, 3.0, 2.0, 0.0, 0.0, 0.0),       # 6 drawn 20 px from its nominal position: fails on max_ashift at bd = 40
    (42.0, 42.0, 0.0, 2.0, 0.0, 0.0, 0.0),       # 7 empty sky (flux 0 draws nothing): an all-zero cut at bd = 4 and 8, the NaN failure
    (2.2, 92.7, 3.5, 2.1, 0.0, 0.05, 0.0),       # 8 (xi, yi) = (2, 93): the cut hangs over two frame edges
    (70.5, 70.4, 2.5, 3.0, -0.2, 0.1, 0.0),     # 9 wide
]
OFFSETS = {5: (-12.0, 0.0), 6: (-20.0, 0.0)}
STAMP = 14  # a star is drawn on the pixels within 14 of its centre's pixel, as an injected stamp: the sky between the stars is exactly zero


def star_positions():
    return np.array([s[0] for s in STARS]), np.array([s[1] for s in STARS])


def draw_star(n, cx, cy, flux, sig, e1, e2, wing):
    """A sampled elliptical Gaussian with moments M = sig^2 / sqrt(1 - e^2) [[1 + e1, e2], [e2, 1 - e1]] (det M = sig^4), plus a fraction
    `wing` of the flux in a (1 + r^2 / (3 sig)^2)^-2 profile."""
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    dx, dy = xx - cx, yy - cy
    f = sig * sig / math.sqrt(1.0 - e1 * e1 - e2 * e2)
    Mxx, Myy, Mxy = f * (1 + e1), f * (1 - e1), f * e2
    det = Mxx * Myy - Mxy * Mxy
    rho2 = (Myy * dx * dx - 2 * Mxy * dx * dy + Mxx * dy * dy) / det
    g = np.exp(-0.5 * rho2) / (2 * math.pi * math.sqrt(det))
    if wing:
        rc2 = (3 * sig) ** 2
        g = (1 - wing) * g + wing / (math.pi * rc2) / (1 + (dx * dx + dy * dy) / rc2) ** 2
    return flux * g


def fixture_frame():
    """The 96 x 96 float32 frame of injected stars and the maps that go with it (deterministic)."""
    frame = np.zeros((N, N))
    for k, (x, y, flux, sig, e1, e2, wing) in enumerate(STARS):
        ox, oy = OFFSETS.get(k, (0.0, 0.0))
        if flux:
            cx, cy = int(np.rint(x + ox)), int(np.rint(y + oy))
            box = np.zeros((N, N), dtype=bool)
            box[max(cy - STAMP, 0):cy + STAMP + 1, max(cx - STAMP, 0):cx + STAMP + 1] = True
            frame += np.where(box, draw_star(N, x + ox, y + oy, flux, sig, e1, e2, wing), 0.0)
    rng = np.random.default_rng(15)
    fid = rng.integers(15000, 30000, (N, N)).astype(np.uint16)  # -10 bels x 10 / code: 30 .. 60 dB
    fid[40:44, 40:60] = 0
    inweight = rng.random((5, N // N2, N // N2)).astype(np.float32) * 0.05
    uc = (10.0 ** rng.uniform(-6, -3, (N, N))).astype(np.float32)
    sigma = rng.uniform(0.2, 0.6, (N, N)).astype(np.float32)
    tsum = rng.uniform(0.9, 1.1, (N, N)).astype(np.float32)
    neff = rng.uniform(2.0, 6.0, (N, N)).astype(np.float32)
    return {"frame": frame.astype(np.float32), "fid": fid, "inweight": inweight, "uc": uc, "sigma": sigma, "tsum": tsum, "neff": neff}
