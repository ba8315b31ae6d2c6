"""Reference for the device HEALPix grids (seam 18), independent of pyimcom_amd: (1) a float64 numpy restatement of the RING scheme of Gorski
et al. 2005 (ApJ 622, 759: pixel centres, section 4.1 with eqs. 2-9, and the inverse) with healpy's argument order -- ``pix2ang``,
``ang2pix``, ``ang2vec``, ``vec2ang``, ``query_disc`` -- so that the module can stand in for ``healpy`` where the reference's statements are
executed; the brute-force cap over a pixel range, the reference-mode range, and the ring-window form of the same cap; (2) the pixel centres
and the cap's ``mu`` in 40-digit arithmetic (mpmath).  healpy is not installed here, so nothing in this file has been compared with healpy."""

import sys

import numpy as np

pixelfunc = sys.modules[__name__]  # ``healpy.pixelfunc.ang2pix`` is ``healpy.ang2pix``
MAX_RES = 29
EPS = np.finfo(np.float64).eps
ANGLE_FLOOR = 3.6e-15  # four units in the last place of 2 pi: a correctly rounded angle cannot beat its representation


def nside2npix(nside):
    return 12 * int(nside) ** 2


def _res(nside):
    n = int(nside)
    assert n >= 1 and n & (n - 1) == 0 and n <= 1 << MAX_RES, nside
    return n.bit_length() - 1


def isqrt(v):
    """floor(sqrt(v)) of int64 values up to 2^63 - 1, exact."""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = r - (r * r > v)
    return r + ((r + 1) * (r + 1) <= v)


def pix2ring(nside, ipix):
    """(ring 1 .. 4 nside - 1, index in ring, quarter of the ring's length, shifted) of RING pixels."""
    n = int(nside)
    p = np.asarray(ipix, dtype=np.int64)
    npix, ncap = 12 * n * n, 2 * n * (n - 1)
    assert np.all((p >= 0) & (p < npix))
    north, south = p < ncap, p >= npix - ncap
    belt = ~(north | south)
    ring, j, quarter, shifted = (np.zeros(p.shape, dtype=np.int64) for _ in range(4))
    i = (1 + isqrt(1 + 2 * p[north])) >> 1
    ring[north], j[north], quarter[north], shifted[north] = i, p[north] - 2 * i * (i - 1), i, 1
    q = p[belt] - ncap
    r = q // (4 * n) + n
    ring[belt], j[belt], quarter[belt], shifted[belt] = r, q % (4 * n), n, ((r - n) & 1) == 0
    i = (1 + isqrt(2 * (npix - p[south]) - 1)) >> 1
    ring[south], j[south], quarter[south], shifted[south] = 4 * n - i, p[south] - (npix - 2 * i * (i + 1)), i, 1
    return ring, j, quarter, shifted


def ring_theta(nside, ring):
    """(theta, z, sin theta) of rings: acos(z), and next to the poles (|z| > 0.99) atan2 from sin(theta) = sqrt(t (2 - t))."""
    n = int(nside)
    ring = np.asarray(ring, dtype=np.int64)
    belt = (ring >= n) & (ring <= 3 * n)
    zb = (2 * n - ring).astype(np.float64) * 2.0 / float(3 * n)
    x = np.where(belt, 0, np.where(ring < n, ring, 4 * n - ring)).astype(np.float64) / float(n)  # (unused in the belt)
    t = x * x / 3.0
    za = 1.0 - t
    zc = np.where(ring < n, za, -za)
    sc = np.sqrt(t * (2.0 - t))
    z = np.where(belt, zb, zc)
    zb = np.where(belt, zb, 0.0)
    sth = np.where(belt, np.sqrt((1.0 - zb) * (1.0 + zb)), sc)
    with np.errstate(invalid="ignore"):
        theta =np.where(belt | (za <= 0.99), np.arccos(np.clip(z, -1.0, 1.0)), np.arctan2(sc, zc))
    return theta, z, sth


def pix2ang(nside, ipix, nest=False, lonlat=False):
    assert not nest
    _res(nside)
    scalar = np.ndim(ipix) == 0
    ring, j, quarter, shifted = pix2ring(nside, np.atleast_1d(ipix))
    theta = ring_theta(nside, ring)[0]
    phi = (j.astype(np.float64) + 0.5 * shifted) / quarter.astype(np.float64) * (np.pi / 2.0)
    a, b = (np.degrees(phi), 90.0 - np.degrees(theta)) if lonlat else (theta, phi)
    return (a[0], b[0]) if scalar else (a, b)


def ang2pix(nside, theta, phi, nest=False, lonlat=False):
    assert not nest
    n = int(nside)
    _res(n)
    scalar = np.ndim(theta) == 0 and np.ndim(phi) == 0
    theta, phi = np.broadcast_arrays(np.atleast_1d(np.asarray(theta, dtype=np.float64)), np.atleast_1d(np.asarray(phi, dtype=np.float64)))
    if lonlat:
        theta, phi = np.pi / 2.0 - np.radians(phi), np.radians(theta)
    assert np.all((theta >= 0) & (theta <= np.pi))
    z = np.cos(theta)
    za = np.abs(z)
    tt = np.mod(phi / (np.pi / 2.0), 4.0)
    tt = np.where(tt < 4.0, tt, 0.0)
    # the belt
    t1, t2 = n * (0.5 + tt), n * z * 0.75
    jp, jm = np.floor(t1 - t2).astype(np.int64), np.floor(t1 + t2).astype(np.int64)
    ir = n + 1 + jp - jm
    kshift = 1 - (ir & 1)
    ip = ((jp + jm - n + kshift + 1 + 8 * n) >> 1) % (4 * n)
    belt = 2 * n * (n - 1) + (ir - 1) * 4 * n + ip
    # the caps
    tp = tt - np.floor(tt)
    tmp = np.where(za < 0.99, n * np.sqrt(3.0 * np.clip(1.0 - za, 0.0, None)), n * np.abs(np.sin(theta)) / np.sqrt((1.0 + za) / 3.0))
    jp, jm = (tp * tmp).astype(np.int64), ((1.0 - tp) * tmp).astype(np.int64)
    ir = np.minimum(jp + jm + 1, n)
    ip = np.minimum((tt * ir).astype(np.int64), 4 * ir - 1)
    caps = np.where(z > 0, 2 * ir * (ir - 1) + ip, 12 * n * n - 2 * ir * (ir + 1) + ip)
    p = np.where(za <= 2.0 / 3.0, belt, caps)
    return int(p[0]) if scalar else p


def ang2vec(theta, phi, lonlat=False):
    if lonlat:
        theta, phi = np.pi / 2.0 - np.radians(phi), np.radians(theta)
    theta, phi = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    st = np.sin(theta)
    return np.stack((st * np.cos(phi), st * np.sin(phi), np.cos(theta)), axis=-1)


def vec2ang(vectors, lonlat=False):
    v = np.asarray(vectors, dtype=np.float64).reshape(-1, 3)
    theta = np.arctan2(np.hypot(v[:, 0], v[:, 1]), v[:, 2])
    phi = np.arctan2(v[:, 1], v[:, 0])
    phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
    return (np.degrees(phi), 90.0 - np.degrees(theta)) if lonlat else (theta, phi)


def cap_mu(ra, dec, theta, phi):
    """The left side of the reference's predicate (layer.py:730-732)."""
    thetac = np.pi / 2.0 - theta
    return np.sin(thetac) * np.sin(dec) + np.cos(thetac) * np.cos(dec) * np.cos(ra - phi)


def reference_range(nside, ra, dec, radius):
    """pmin, pmax of layer.py:721-725."""
    radext = radius + 3 / nside
    dmin = max(dec - radext, -np.pi / 2.0)
    dmax = min(dec + radext, np.pi / 2.0)
    return ang2pix(nside, np.pi / 2.0 - dmax, ra), ang2pix(nside, np.pi / 2.0 - dmin, ra)


def disc_range(nside, ra, dec, radius):
    """The whole rings of the reference range: every pixel of the disc lies inside (3 / nside is more than three rings)."""
    pmin, pmax = reference_range(nside, ra, dec, radius)
    ring, j, quarter, _ = pix2ring(nside, np.array([pmin, pmax]))
    return int(pmin - j[0]), int(pmax - j[1] + 4 * quarter[1] - 1)


def cap_brute(nside, ra, dec, radius, pmin, pmax, chunk=1 << 22):
    """(ipix, theta, phi, smallest |mu - cos r| over the candidates) of the pixels pmin .. pmax with mu >= cos(radius), every pixel tested."""
    keep, near = [], np.inf
    c = np.cos(radius)
    for lo in range(int(pmin), int(pmax) + 1, chunk):
        p = np.arange(lo, min(lo + chunk, int(pmax) + 1), dtype=np.int64)
        theta, phi = pix2ang(nside, p)
        mu = cap_mu(ra, dec, theta, phi)
        near = min(near, float(np.min(np.abs(mu - c)))) if p.size else near
        good = mu >= c
        keep.append((p[good], theta[good], phi[good]))
    return tuple(np.concatenate([k[i] for k in keep]) for i in range(3)) + (near,)


def query_disc(nside, vec, radius, inclusive=False, nest=False):
    """The ascending pixels whose centres lie within ``radius`` of ``vec`` (every pixel of the rings in reach is tested)."""
    assert not nest and not inclusive
    theta, phi = vec2ang(vec)
    ra, dec = float(phi[0]), float(np.pi / 2.0 - theta[0])
    return cap_brute(nside, ra, dec, radius, *disc_range(nside, ra, dec, radius))[0]


def ring_window(theta, sth, theta0, s0, radius, ra, length, shifted):
    """(first, count) of csrc/healpix_core.h's hp_ring_window for one ring."""
    d = theta - theta0
    ad = abs(d)
    if ad > radius * (1.0 + 1e-12) + 1e-15:
        return 0, 0
    den = sth * s0
    h = np.sin(0.5 * (radius + d)) * np.sin(0.5 * (radius - d)) if radius > ad else 0.0
    if not den > 0.0 or not h < den:
        return 0, length
    dphi, step, off = 2.0 * np.arcsin(np.sqrt(h / den)), 2.0 * np.pi / length, 0.5 if shifted else 0.0
    lo, hi = int(np.floor((ra - dphi) / step - off)) - 1, int(np.ceil((ra + dphi) / step - off)) + 1
    if hi - lo + 1 >= length:
        return 0, length
    return lo % length, hi - lo + 1


def cap_windowed(nside, ra, dec, radius, full_disc=False):
    """The cap ring by ring through the phi windows, ascending: (ipix, theta, phi, candidates tested)."""
    n = int(nside)
    pmin, pmax = reference_range(n, ra, dec, radius)
    plo, phi_ = disc_range(n, ra, dec, radius) if full_disc else (pmin, pmax)
    r0, r1 = (int(r) for r in pix2ring(n, np.array([pmin, pmax]))[0])
    c, theta0, s0, raw = np.cos(radius), np.pi / 2.0 - dec, max(np.cos(dec), 0.0), float(np.mod(ra, 2.0 * np.pi))
    rings = np.arange(r0, r1 + 1)
    thetas, _, sths = ring_theta(n, rings)
    keep, tested = [], 0
    for ring, theta, sth in zip(rings, thetas, sths):
        quarter = ring if ring < n else (n if ring <= 3 * n else 4 * n - ring)
        start = 2 * ring * (ring - 1) if ring < n else (2 * n * (n - 1) + (ring - n) * 4 * n if ring <= 3 * n else 12 * n * n - 2 * quarter * (quarter + 1))
        shifted = 1 if (ring < n or ring > 3 * n) else int(((ring - n) & 1) == 0)
        first, count = ring_window(theta, sth, theta0, s0, radius, raw, 4 * quarter, shifted)
        nlow = max(first + count - 4 * quarter, 0)
        j = np.concatenate((np.arange(nlow), np.arange(first, first + count - nlow))).astype(np.int64)
        p = start + j
        inside = (p >= plo) & (p <= phi_)
        j, p = j[inside], p[inside]
        tested += p.size
        phi = (j.astype(np.float64) + 0.5 * shifted) / float(quarter) * (np.pi / 2.0)
        good = cap_mu(ra, dec, theta, phi) >= c
        keep.append((p[good], np.full(int(good.sum()), theta), phi[good]))
    return tuple(np.concatenate([k[i] for k in keep]) for i in range(3)) + (tested,)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (2) 40-digit arithmetic

def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def mp_pix2ang(nside, p):
    """(theta, phi) of one pixel as 40-digit numbers, ring and index from Python integers."""
    import math

    mp = _mp()
    n, p = int(nside), int(p)
    npix, ncap = 12 * n * n, 2 * n * (n - 1)
    assert 0 <= p < npix
    if p < ncap:
        i = (1 + math.isqrt(1 + 2 * p)) >> 1
        j, z, s, q = p - 2 * i * (i - 1), 1 - mp.mpf(i * i) / (3 * n * n), mp.mpf(1) / 2, i
    elif p < npix - ncap:
        ring, j = (p - ncap) // (4 * n) + n, (p - ncap) % (4 * n)
        z, s, q = mp.mpf(2 * (2 * n - ring)) / (3 * n), (mp.mpf(1) / 2 if (ring - n) % 2 == 0 else mp.mpf(0)), n
    else:
        i = (1 + math.isqrt(2 * (npix - p) - 1)) >> 1
        j, z, s, q = p - (npix - 2 * i * (i + 1)), -(1 - mp.mpf(i * i) / (3 * n * n)), mp.mpf(1) / 2, i
    return mp.atan2(mp.sqrt((1 - z) * (1 + z)), z), (j + s) * mp.pi / (2 * q)


def mp_cap_mu(ra, dec, theta, phi):
    """mu of the float64 centre (ra, dec) and a 40-digit pixel centre."""
    mp = _mp()
    ra, dec = mp.mpf(float(ra)), mp.mpf(float(dec))
    return mp.cos(theta) * mp.sin(dec) + mp.sin(theta) * mp.cos(dec) * mp.cos(ra - phi)
