"""Reference for the device WCS (seam 16), independent of pyimcom_amd: (1) a float64 numpy restatement of the arithmetic that csrc/wcs_core.h
states -- SIP by Horner, CD, the zenithal projections TAN and STG as unit vectors, the rotation of the sphere, the Newton inverse of the SIP,
the bilinear error map with linear extrapolation and the fixed-point steps of the inverse -- working from a packed descriptor; (2) the
published definitions (FITS WCS paper II, Calabretta & Greisen 2002, eqs. 2, 5, 54-56 with their trigonometry; the SIP convention, Shupe et
al. 2005) evaluated from the HEADER VALUES in 40-digit arithmetic (mpmath).  astropy is not installed here, so nothing in this file has been
compared with astropy / wcslib.

The 40-digit chain never sees the descriptor: its rotation is the trigonometry of eq. (2) itself, so a wrong matrix in the packer or in the
core shows as a difference.  Error tables are data (exact binary values) in both."""

import numpy as np

TAN, STG = 0, 1
MAX_ORDER = 9
NCOEF = 55
D_PROJ, D_CRPIX, D_CD, D_ROT, D_AORDER, D_BORDER, D_NITER, D_A = 0, 1, 3, 7, 16, 17, 18, 20
D_B = D_A + NCOEF
DESC_LEN = D_B + NCOEF
NEWTON_CAP, NEWTON_TOL = 12, 2.0 ** -40
DEG = np.pi / 180.0
RAD = 180.0 / np.pi
EPS = np.finfo(np.float64).eps


def sip_index(p, q):
    return p * 10 - p * (p - 1) // 2 + q


# ---------------------------------------------------------------------------------------------------------------------------------------
# headers -> plain parameters (both chains read a header through this)

def header_params(h):
    """dict(proj, crpix, crval, cd, lonpole, a, b) of a header-like dict; a, b: {(p, q): value}."""
    ctype = h["CTYPE1"].strip()[5:]
    proj = {"TAN": TAN, "TAN-SIP": TAN, "STG": STG}[ctype]
    if "CD1_1" in h:
        cd = [h.get(k, 0.0) for k in ("CD1_1", "CD1_2", "CD2_1", "CD2_2")]
    else:
        pc = [h.get("PC1_1", 1.0), h.get("PC1_2", 0.0), h.get("PC2_1", 0.0), h.get("PC2_2", 1.0)]
        cd = [h["CDELT1"] * pc[0], h["CDELT1"] * pc[1], h["CDELT2"] * pc[2], h["CDELT2"] * pc[3]]
    lonpole = h.get("LONPOLE", 0.0 if h["CRVAL2"] == 90.0 else 180.0)
    ab = []
    for L in "AB":
        order = int(h.get(f"{L}_ORDER", 0))
        ab.append({(p, q): float(h.get(f"{L}_{p}_{q}", 0.0)) for p in range(order + 1) for q in range(order + 1 - p)})
    return dict(proj=proj, crpix=[float(h["CRPIX1"]), float(h["CRPIX2"])], crval=[float(h["CRVAL1"]), float(h["CRVAL2"])], cd=[float(v) for v in cd],
                lonpole=float(lonpole), a=ab[0], b=ab[1], a_order=int(h.get("A_ORDER", 0)), b_order=int(h.get("B_ORDER", 0)))


def pixel_scale_rad(desc):
    cd = desc[D_CD:D_CD + 4]
    return np.sqrt(abs(cd[0] * cd[3] - cd[1] * cd[2])) * DEG


# ---------------------------------------------------------------------------------------------------------------------------------------
# (1) float64 numpy restatement, from the packed descriptor

def np_sip(c, order, u, v):
    """f, df/du, df/dv of sum c_pq u^p v^q: Horner in v inside Horner in u."""
    F = np.zeros_like(u)
    Fu = np.zeros_like(u)
    Fv = np.zeros_like(u)
    for p in range(order, -1, -1):
        g = np.zeros_like(u)
        gv = np.zeros_like(u)
        for q in range(order - p, -1, -1):
            gv = gv * v + g
            g = g * v + c[sip_index(p, q)]
        Fu = Fu * u + F
        F = F * u + g
        Fv = Fv * u + gv
    return F, Fu, Fv


def np_cell(t, n2, lo, hi):
    """(cell index, normalised distance) on the axis lo, 0, 1, .., N - 1, hi."""
    N = n2 - 2
    nodes = np.concatenate(([lo], np.arange(N, dtype=np.float64), [hi]))
    i = np.where(t < 0, 0, np.where(t >= N - 1, N, 1 + np.floor(np.clip(t, 0, N - 1)).astype(np.int64)))
    i = np.clip(i, 0, N)
    return i, (t - nodes[i]) / (nodes[i + 1] - nodes[i])


def np_table(tab, x, y):
    """(dx, dy) at the points (x, y): tab = (values [2, n2, n2], lo, hi), axes (y, x); float64 accumulation, scipy's term order."""
    values, lo, hi = tab
    n2 = values.shape[1]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    bad = ~(np.isfinite(x) & np.isfinite(y))
    ix, fx = np_cell(np.where(bad, 0.0, x), n2, lo, hi)
    iy, fy = np_cell(np.where(bad, 0.0, y), n2, lo, hi)
    out = []
    for k in (0, 1):
        v = values[k].astype(np.float64)
        s = v[iy, ix] * ((1 - fy) * (1 - fx))
        s = s + v[iy, ix + 1] * ((1 - fy) * fx)
        s = s + v[iy + 1, ix] * (fy * (1 - fx))
        s = s + v[iy + 1, ix + 1] * (fy * fx)
        out.append(np.where(bad, np.nan, s))
    return out[0], out[1]


def np_pix2native(d, tab, x, y, origin):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if tab is not None:
        dx, dy = np_table(tab, x, y)
        x, y = x + dx, y + dy
    u = x + (1 - origin) - d[D_CRPIX]
    v = y + (1 - origin) - d[D_CRPIX + 1]
    up, vp = u, v
    ao, bo = int(d[D_AORDER]), int(d[D_BORDER])
    if ao:
        up = u + np_sip(d[D_A:D_A + NCOEF], ao, u, v)[0]
    if bo:
        vp = v + np_sip(d[D_B:D_B + NCOEF], bo, u, v)[0]
    xi = (d[D_CD] * up + d[D_CD + 1] * vp) * DEG
    eta = (d[D_CD + 2] * up + d[D_CD + 3] * vp) * DEG
    r2 = xi * xi + eta * eta
    if int(d[D_PROJ]) == TAN:
        s = 1.0 / np.sqrt(1.0 + r2)
        return np.stack((-eta * s, xi * s, s))
    s = 1.0 / (4.0 + r2)
    return np.stack((-4.0 * eta * s, 4.0 * xi * s, (4.0 - r2) * s))


def np_native2pix(d, tab, n, origin):
    """(x, y, ok): NaN where not ok."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(n).all(axis=0)
        if int(d[D_PROJ]) == TAN:
            ok = fin & (n[2] > 0)
            xi, eta = n[1] / n[2], -n[0] / n[2]
        else:
            s = 1.0 + n[2]
            ok = fin & (s > 0)
            xi, eta = 2.0 * n[1] / s, -2.0 * n[0] / s
        ok = ok & np.isfinite(xi) & np.isfinite(eta)
        xi, eta = np.where(ok, xi, 0.0) * RAD, np.where(ok, eta, 0.0) * RAD
        c11, c12, c21, c22 = d[D_CD:D_CD + 4]
        det = c11 * c22 - c12 * c21
        U, V = (c22 * xi - c12 * eta) / det, (c11 * eta - c21 * xi) / det
        u, v = U.copy(), V.copy()
        ao, bo = int(d[D_AORDER]), int(d[D_BORDER])
        if ao or bo:
            stopped = np.zeros(u.shape, dtype=bool)
            zero = (np.zeros_like(u),) * 3
            for _ in range(NEWTON_CAP):
                a, au, av = np_sip(d[D_A:D_A + NCOEF], ao, u, v) if ao else zero
                b, bu, bv = np_sip(d[D_B:D_B + NCOEF], bo, u, v) if bo else zero
                f1, f2 = (u - U) + a, (v - V) + b
                j11, j22 = 1.0 + au, 1.0 + bv
                jd = j11 * j22 - av * bu
                du, dv = (j22 * f1 - av * f2) / jd, (j11 * f2 - bu * f1) / jd
                u, v = np.where(stopped, u, u - du), np.where(stopped, v, v - dv)
                # a step below 2^-40 pixel, or below 2^-52 of the coordinate where that is more (beyond 4096 pixels an ulp exceeds 2^-40)
                stopped = stopped | ((np.abs(du) < np.maximum(NEWTON_TOL, EPS * np.abs(u))) & (np.abs(dv) < np.maximum(NEWTON_TOL, EPS * np.abs(v))))
                if stopped.all():
                    break
            ok = ok & stopped
        x2 = np.where(ok, u + d[D_CRPIX] - (1 - origin), np.nan)
        y2 = np.where(ok, v + d[D_CRPIX + 1] - (1 - origin), np.nan)
        x1, y1 = x2, y2
        if tab is not None:
            for _ in range(int(d[D_NITER])):
                dx, dy = np_table(tab, x1, y1)
                x1, y1 = x2 - dx, y2 - dy
    return x1, y1, ok


def np_pix2world(d, tab, x, y, origin=0):
    n = np_pix2native(d, tab, x, y, origin)
    R = d[D_ROT:D_ROT + 9].reshape(3, 3)
    c = np.stack([R[0, k] * n[0] + R[1, k] * n[1] + R[2, k] * n[2] for k in range(3)])
    ra = np.arctan2(c[1], c[0]) * RAD
    ra = np.where(ra < 0, ra + 360.0, ra)
    ra = np.where(ra >= 360.0, 0.0, ra)
    return ra, np.arctan2(c[2], np.hypot(c[0], c[1])) * RAD


def np_world2pix(d, tab, ra, dec, origin=0):
    a, de = np.asarray(ra, dtype=np.float64) * DEG, np.asarray(dec, dtype=np.float64) * DEG
    c = np.stack((np.cos(de) * np.cos(a), np.cos(de) * np.sin(a), np.sin(de)))
    R = d[D_ROT:D_ROT + 9].reshape(3, 3)
    n = np.stack([R[k, 0] * c[0] + R[k, 1] * c[1] + R[k, 2] * c[2] for k in range(3)])
    return np_native2pix(d, tab, n, origin)


def np_pix2pix(df, tf, dt, tt, x, y, origin=0):
    nf = np_pix2native(df, tf, x, y, origin)
    Rf, Rt = df[D_ROT:D_ROT + 9].reshape(3, 3), dt[D_ROT:D_ROT + 9].reshape(3, 3)
    M = np.array([[sum(Rt[i, k] * Rf[j, k] for k in range(3)) for j in range(3)] for i in range(3)])
    nt = np.stack([M[k, 0] * nf[0] + M[k, 1] * nf[1] + M[k, 2] * nf[2] for k in range(3)])
    return np_native2pix(dt, tt, nt, origin)


def is_in_ref(xf, yf, nside, pad):
    """compareutils.py:103-105, as numpy evaluates it."""
    with np.errstate(invalid="ignore"):
        return np.logical_and((xf + 0.5 + pad) * (nside - 0.5 - xf + pad) > 0, (yf + 0.5 + pad) * (nside - 0.5 - yf + pad) >= 0)


def grid_axis(nside, pad, subsamp):
    """The pixel coordinates of map_sca2sca's grid along one axis: every subsamp-th of -pad .. nside - 1 + pad, from index subsamp // 2."""
    first, step = (subsamp // 2, subsamp) if subsamp > 1 else (0, 1)
    return np.arange(first, nside + 2 * pad, step).astype(np.float64) - pad


def np_map_sca2sca(dtgt, ttgt, dref, tref, nside, pad=0, subsamp=1):
    s = grid_axis(nside, pad, subsamp)
    xi, yi = np.meshgrid(s, s)
    xf, yf, _ = np_pix2pix(dtgt, ttgt, dref, tref, xi, yi, 0)
    return xf, yf, is_in_ref(xf, yf, nside, pad)


def unit_vectors(ra, dec):
    a, d = np.deg2rad(ra), np.deg2rad(dec)
    return np.stack((np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)), axis=-1)


def np_cap(d, tab, nside, pad):
    """(centre unit vector, 1 - cos of the angle to the farthest padded corner) of a chip."""
    corners = np.array([[sx, sy] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)])
    pix = (nside - 1.0) / 2.0 + (nside / 2.0 + pad) * np.vstack(([[0.0, 0.0]], corners))
    v = unit_vectors(*np_pix2world(d, tab, pix[:, 0], pix[:, 1], 0))
    return v[0], float(np.max(1.0 - v[1:] @ v[0]))


def np_overlap_matrix(descs, nside, pad=0, subsamp=1):
    """float32 [N, N]: 1 on the diagonal, 0 where the caps of two chips cannot touch (centre angle >= sum of the radii), else the fraction
    of chip i's grid inside chip j for i > j, mirrored."""
    caps = [np_cap(d, None, nside, float(pad)) for d in descs]
    centres = np.array([c[0] for c in caps])
    cos_t = 1.0 - np.array([c[1] for c in caps])
    sin_t = np.sqrt(np.clip(1.0 - cos_t * cos_t, 0.0, None))
    touch = centres @ centres.T > np.outer(cos_t, cos_t) - np.outer(sin_t, sin_t)
    ov = touch.astype(np.float32)
    for i, j in zip(*np.nonzero(np.tril(touch, -1))):
        m = np_map_sca2sca(descs[i], None, descs[j], None, nside, pad, subsamp)[2]
        ov[i, j] = ov[j, i] = np.float32(np.count_nonzero(m) / m.size)
    return ov


def area_axis(lo, hi, pad, ovsamp):
    """Centres of the ovsamp sub-pixels of the pixels lo - pad .. hi + pad - 1."""
    half = 0.5 / ovsamp
    return np.linspace(lo - 0.5 + half - pad, hi - 0.5 - half + pad, ovsamp * (hi - lo + 2 * pad))


def area_axes(region, pad, ovsamp):
    return area_axis(region[0], region[1], pad, ovsamp), area_axis(region[2], region[3], pad, ovsamp)


def turned_frame(ra, dec):
    """(ra, dec) in the frame whose pole is the old y axis and whose ra = 180 is the old x axis: far from ra = 0 for a footprint there."""
    c = unit_vectors(ra, dec)
    return np.arctan2(-c[..., 2], c[..., 0]) / DEG + 180.0, np.arcsin(c[..., 1]) / DEG


def np_pix_area(d, tab, region, pad=1, ovsamp=1):
    """The pixel areas as wcsutil.get_pix_area defines them, in float64: centred differences of ra and dec in degrees over 2 pad pixels, the
    determinant, cos(dec); a footprint wider than 45 degrees in ra is turned first.  (area, whether it was turned)."""
    xs, ys = area_axes(region, pad, ovsamp)
    xi, yi = np.meshgrid(xs, ys)
    ra, dec = np_pix2world(d, tab, xi, yi, 0)
    turned = bool(ra.max() - ra.min() > 45.0)
    if turned:
        ra, dec = turned_frame(ra, dec)
    op = ovsamp * pad
    inner = slice(op, -op)

    def ddx(f):
        return (f[inner, 2 * op:] - f[inner, :-2 * op]) / 2 / pad

    def ddy(f):
        return (f[2 * op:, inner] - f[:-2 * op, inner]) / 2 / pad

    return np.abs(ddx(ra) * ddy(dec) - ddy(ra) * ddx(dec)) * np.cos(dec[inner, inner] * DEG), turned


# ---------------------------------------------------------------------------------------------------------------------------------------
# (2) the definitions in 40-digit arithmetic, from the header values

def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def mp_table(tab, x, y):
    mp = _mp()
    values, lo, hi = tab
    n2 = values.shape[1]
    N = n2 - 2

    def cell(t):
        i = 0 if t < 0 else (N if t >= N - 1 else 1 + int(mp.floor(t)))
        node = lambda k: mp.mpf(lo) if k == 0 else (mp.mpf(hi) if k == n2 - 1 else mp.mpf(k - 1))  # noqa: E731
        return i, (t - node(i)) / (node(i + 1) - node(i))

    ix, fx = cell(x)
    iy, fy = cell(y)
    out = []
    for k in (0, 1):
        v = values[k]
        out.append(mp.mpf(float(v[iy, ix])) * (1 - fy) * (1 - fx) + mp.mpf(float(v[iy, ix + 1])) * (1 - fy) * fx
                   + mp.mpf(float(v[iy + 1, ix])) * fy * (1 - fx) + mp.mpf(float(v[iy + 1, ix + 1])) * fy * fx)
    return out[0], out[1]


def _mp_poly(c, u, v):
    return sum((_mp().mpf(val) * u ** p * v ** q for (p, q), val in c.items()), _mp().mpf(0))


def _mp_dpoly(c, u, v):
    mp = _mp()
    fu = sum((mp.mpf(val) * p * u ** (p - 1) * v ** q for (p, q), val in c.items() if p > 0), mp.mpf(0))
    fv = sum((mp.mpf(val) * q * u ** p * v ** (q - 1) for (p, q), val in c.items() if q > 0), mp.mpf(0))
    return fu, fv


def mp_pix2native(P, tab, x, y, origin):
    """(phi, theta) in radians (Paper II eqs. 14-15 with 54-55: TAN R = (180/pi) cot theta, STG R = (360/pi) tan((90 - theta) / 2))."""
    mp = _mp()
    x, y = mp.mpf(float(x)), mp.mpf(float(y))
    if tab is not None:
        dx, dy = mp_table(tab, x, y)
        x, y = x + dx, y + dy
    u, v = x + (1 - origin) - mp.mpf(P["crpix"][0]), y + (1 - origin) - mp.mpf(P["crpix"][1])
    up, vp = u + _mp_poly(P["a"], u, v), v + _mp_poly(P["b"], u, v)
    cd = [mp.mpf(c) for c in P["cd"]]
    xi, eta = cd[0] * up + cd[1] * vp, cd[2] * up + cd[3] * vp  # degrees
    phi = mp.atan2(xi, -eta)
    Rt = mp.sqrt(xi * xi + eta * eta) * mp.pi / 180
    theta = mp.atan2(1, Rt) if P["proj"] == TAN else mp.pi / 2 - 2 * mp.atan(Rt / 2)
    return phi, theta


def mp_native2pix(P, tab, niter, phi, theta, origin):
    mp = _mp()
    if P["proj"] == TAN:
        Rt = mp.cos(theta) / mp.sin(theta)
    else:
        Rt = 2 * mp.cos(theta) / (1 + mp.sin(theta))
    Rt = Rt * 180 / mp.pi
    xi, eta = Rt * mp.sin(phi), -Rt * mp.cos(phi)
    cd = [mp.mpf(c) for c in P["cd"]]
    det = cd[0] * cd[3] - cd[1] * cd[2]
    U, V = (cd[3] * xi - cd[1] * eta) / det, (cd[0] * eta - cd[2] * xi) / det
    u, v = U, V
    if P["a"] or P["b"]:
        for _ in range(60):
            f1, f2 = u + _mp_poly(P["a"], u, v) - U, v + _mp_poly(P["b"], u, v) - V
            au, av = _mp_dpoly(P["a"], u, v)
            bu, bv = _mp_dpoly(P["b"], u, v)
            jd = (1 + au) * (1 + bv) - av * bu
            du, dv = ((1 + bv) * f1 - av * f2) / jd, ((1 + au) * f2 - bu * f1) / jd
            u, v = u - du, v - dv
            if abs(du) < mp.mpf(10) ** -35 and abs(dv) < mp.mpf(10) ** -35:
                break
        else:
            raise RuntimeError("the 40-digit Newton iteration did not converge")
    x2, y2 = u + mp.mpf(P["crpix"][0]) - (1 - origin), v + mp.mpf(P["crpix"][1]) - (1 - origin)
    x1, y1 = x2, y2
    if tab is not None:
        for _ in range(niter):
            dx, dy = mp_table(tab, x1, y1)
            x1, y1 = x2 - dx, y2 - dy
    return x1, y1


def mp_native2world(P, phi, theta):
    """Paper II eq. (2): (alpha, delta) in radians."""
    mp = _mp()
    ap, dp, pp = (mp.mpf(v) * mp.pi / 180 for v in (P["crval"][0], P["crval"][1], P["lonpole"]))
    dphi = phi - pp
    alpha = ap + mp.atan2(-mp.cos(theta) * mp.sin(dphi), mp.sin(theta) * mp.cos(dp) - mp.cos(theta) * mp.sin(dp) * mp.cos(dphi))
    st = mp.sin(theta) * mp.sin(dp) + mp.cos(theta) * mp.cos(dp) * mp.cos(dphi)
    ct = mp.hypot(mp.cos(theta) * mp.sin(dphi), mp.sin(theta) * mp.cos(dp) - mp.cos(theta) * mp.sin(dp) * mp.cos(dphi))
    return alpha, mp.atan2(st, ct)


def mp_world2native(P, alpha, delta):
    """Paper II eq. (5)."""
    mp = _mp()
    ap, dp, pp = (mp.mpf(v) * mp.pi / 180 for v in (P["crval"][0], P["crval"][1], P["lonpole"]))
    da = alpha - ap
    y_, x_ = -mp.cos(delta) * mp.sin(da), mp.sin(delta) * mp.cos(dp) - mp.cos(delta) * mp.sin(dp) * mp.cos(da)
    phi = pp + mp.atan2(y_, x_)
    theta = mp.atan2(mp.sin(delta) * mp.sin(dp) + mp.cos(delta) * mp.cos(dp) * mp.cos(da), mp.hypot(x_, y_))
    return phi, theta


def mp_pix2world(P, tab, x, y, origin=0):
    """(ra in [0, 360), dec) in degrees, as 40-digit numbers."""
    mp = _mp()
    alpha, delta = mp_native2world(P, *mp_pix2native(P, tab, x, y, origin))
    ra = alpha * 180 / mp.pi
    ra = ra - 360 * mp.floor(ra / 360)
    return ra, delta * 180 / mp.pi


def mp_world2pix(P, tab, niter, ra, dec, origin=0):
    mp = _mp()
    phi, theta = mp_world2native(P, mp.mpf(float(ra)) * mp.pi / 180, mp.mpf(float(dec)) * mp.pi / 180)
    return mp_native2pix(P, tab, niter, phi, theta, origin)


def mp_pix2pix(Pf, tf, Pt, tt, niter, x, y, origin=0):
    alpha, delta = mp_native2world(Pf, *mp_pix2native(Pf, tf, x, y, origin))
    phi, theta = mp_world2native(Pt, alpha, delta)
    return mp_native2pix(Pt, tt, niter, phi, theta, origin)


def mp_pix_area(P, tab, region, pad=1, ovsamp=1):
    """get_pix_area's formula with every step in 40 digits (the axes are numpy's linspace values, taken as exact)."""
    mp = _mp()
    xs, ys = area_axes(region, pad, ovsamp)
    W, H = len(xs), len(ys)
    ra = [[None] * W for _ in range(H)]
    dec = [[None] * W for _ in range(H)]
    for j in range(H):
        for i in range(W):
            ra[j][i], dec[j][i] = mp_pix2world(P, tab, xs[i], ys[j], 0)
    flat = [v for row in ra for v in row]
    if max(flat) - min(flat) > 45:
        deg = mp.pi / 180
        for j in range(H):
            for i in range(W):
                a, d = ra[j][i] * deg, dec[j][i] * deg
                cx, cy, cz = mp.cos(d) * mp.cos(a), mp.cos(d) * mp.sin(a), mp.sin(d)
                dec[j][i] = mp.asin(cy) / deg
                ra[j][i] = mp.atan2(-cz, cx) / deg + 180
    op = ovsamp * pad
    out = np.zeros((H - 2 * op, W - 2 * op))
    for j in range(H - 2 * op):
        for i in range(W - 2 * op):
            rx = (ra[j + op][i + 2 * op] - ra[j + op][i]) / 2 / pad
            ry = (ra[j + 2 * op][i + op] - ra[j][i + op]) / 2 / pad
            dx = (dec[j + op][i + 2 * op] - dec[j + op][i]) / 2 / pad
            dy = (dec[j + 2 * op][i + op] - dec[j][i + op]) / 2 / pad
            out[j, i] = float(abs(rx * dy - ry * dx) * mp.cos(dec[j + op][i + op] * mp.pi / 180))
    return out


def ra_distance(a, b):
    """|a - b| on the circle, degrees."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.minimum(d, 360.0 - d)
