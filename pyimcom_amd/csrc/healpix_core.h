// healpix_core.h -- the per-pixel arithmetic of the HEALPix kernels of wcs.hip: the RING scheme of Gorski et al. 2005 (ApJ 622, 759; pixel
// centres: section 4.1, eqs. 2-9, and their inverse) for nside = 2^res, res 0 .. 29, with int64 pixel indices, and the spherical cap of the
// reference's GridInject.make_sph_grid (src/pyimcom/layer.py:690-740).  A ring is numbered 1 .. 4 nside - 1 from the north pole; a pixel is
// (ring, index in ring).  One pixel has one owner and nothing is reduced.  Compiles as host code too (tests/native/healpix_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HP_HD __host__ __device__ __forceinline__
#else
#define HP_HD inline
#endif
// The statements that are compared with numpy's bit for bit are kept as numpy evaluates them: every product and sum rounded on its own.
#if defined(__clang__)
#define HP_SEPARATE_ROUNDINGS _Pragma("clang fp contract(off)")
#else
#define HP_SEPARATE_ROUNDINGS
#endif

namespace imcom {

constexpr int HP_MAX_RES = 29;
constexpr double HP_PI = 3.141592653589793, HP_HALFPI = 1.5707963267948966, HP_TWOPI = 6.283185307179586;
constexpr double HP_DEG = 0.017453292519943295;     // pi / 180, the reference's `degree`
constexpr double HP_PER_RAD = 57.29577951308232;    // 180 / pi, the factor of numpy's degrees()
constexpr double HP_TWOTHIRD = 2.0 / 3.0;

struct HpRing {
    int64_t ring, start, len;  // 1 .. 4 nside - 1; the ring's first pixel; its pixels
    int64_t quarter;           // len / 4: the ring's number within its cap, nside in the belt
    int shifted;               // 1: the centres are at (j + 1/2) steps of 2 pi / len, 0: at j steps
};

// floor(sqrt(v)), exact: the double root and an integer correction (v up to 2 * 12 * 4^29 < 2^63).
HP_HD uint64_t hp_isqrt(uint64_t v)
{
    uint64_t r = (uint64_t)sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

HP_HD int64_t hp_nside(int res) { return (int64_t)1 << res; }
HP_HD int64_t hp_npix(int res) { return (int64_t)12 << (2 * res); }
HP_HD int64_t hp_ncap(int res) { return 2 * hp_nside(res) * (hp_nside(res) - 1); }

// The ring of pixel p (0 <= p < npix).
HP_HD int64_t hp_pix2ring(int res, int64_t p)
{
    const int64_t n = hp_nside(res), ncap = hp_ncap(res), npix = hp_npix(res);
    if (p < ncap) return (int64_t)((1 + hp_isqrt((uint64_t)(1 + 2 * p))) >> 1);
    if (p < npix - ncap) return (p - ncap) / (4 * n) + n;
    return 4 * n - (int64_t)((1 + hp_isqrt((uint64_t)(2 * (npix - p) - 1))) >> 1);
}

// Start, length and shift of ring r: north cap, equatorial belt, south cap.
HP_HD void hp_ring_info(int res, int64_t r, HpRing *g)
{
    const int64_t n = hp_nside(res);
    g->ring = r;
    if (r < n) {
        g->start = 2 * r * (r - 1), g->quarter = r, g->shifted = 1;
    } else if (r <= 3 * n) {
        g->start = hp_ncap(res) + (r - n) * 4 * n, g->quarter = n, g->shifted = ((r - n) & 1) == 0;
    } else {
        const int64_t i = 4 * n - r;
        g->start = hp_npix(res) - 2 * i * (i + 1), g->quarter = i, g->shifted = 1;
    }
    g->len = 4 * g->quarter;
}

// The colatitude of ring r with z = cos(theta) and sin(theta).  In the caps z = +-(1 - t), t = i^2 / (3 nside^2); within |z| > 0.99 the
// colatitude comes from sin(theta) = sqrt(t (2 - t)) -- acos(z) loses half the digits next to a pole.
HP_HD double hp_ring_theta(int res, int64_t r, double *z, double *sth)
{
    const int64_t n = hp_nside(res);
    if (r >= n && r <= 3 * n) {
        const double zz = (double)(2 * n - r) * 2.0 / (double)(3 * n);
        *z = zz, *sth = sqrt((1.0 - zz) * (1.0 + zz));
        return acos(zz);
    }
    const bool north = r < n;
    const double x = (double)(north ? r : 4 * n - r) / (double)n;  // (exact: nside is a power of two)
    const double t = x * x / 3.0, za = 1.0 - t, s = sqrt(t * (2.0 - t));
    *z = north ? za : -za, *sth = s;
    if (za > 0.99) return atan2(s, *z);
    return acos(*z);
}

// The longitude of the pixel of index j in its ring.
HP_HD double hp_ring_phi(const HpRing &g, int64_t j) { return ((double)j + (g.shifted ? 0.5 : 0.0)) / (double)g.quarter * HP_HALFPI; }

// Pixel -> centre (theta, phi) in radians.
HP_HD void hp_pix2ang(int res, int64_t p, double *theta, double *phi)
{
    HpRing g;
    hp_ring_info(res, hp_pix2ring(res, p), &g);
    double z, s;
    *theta = hp_ring_theta(res, g.ring, &z, &s);
    *phi = hp_ring_phi(g, p - g.start);
}

// numpy's degrees(phi) and 90 - degrees(theta) (healpy's lonlat), or (lonlat 0) the reference's rapix / degree and decpix / degree with
// decpix = pi / 2 - theta (layer.py:730, 787-789): one IEEE division each.
HP_HD void hp_degrees(double theta, double phi, int lonlat, double *lon, double *lat)
{
    HP_SEPARATE_ROUNDINGS
    if (lonlat) {
        const double t = theta * HP_PER_RAD;
        *lon = phi * HP_PER_RAD, *lat = 90.0 - t;
    } else {
        const double d = HP_HALFPI - theta;
        *lon = phi / HP_DEG, *lat = d / HP_DEG;
    }
}

// v reduced into [0, w), w > 0.
HP_HD double hp_fmodulo(double v, double w)
{
    if (v >= 0.0) return v < w ? v : fmod(v, w);
    const double t = fmod(v, w) + w;
    return t == w ? 0.0 : t;
}

// (theta, phi) -> pixel: the belt |z| <= 2/3 and the caps; phi may be any finite angle, theta is in [0, pi].
HP_HD int64_t hp_ang2pix(int res, double theta, double phi)
{
    const int64_t n = hp_nside(res), nl4 = 4 * n;
    const double z = cos(theta), za = fabs(z);
    double tt = hp_fmodulo(phi / HP_HALFPI, 4.0);  // in [0, 4)
    if (!(tt < 4.0)) tt = 0.0;
    if (za <= HP_TWOTHIRD) {
        const double t1 = (double)n * (0.5 + tt), t2 = (double)n * z * 0.75;
        const int64_t jp = (int64_t)floor(t1 - t2), jm = (int64_t)floor(t1 + t2);  // the ascending and the descending edge line
        const int64_t ir = n + 1 + jp - jm;                                        // 1 .. 2 n + 1, counted from z = 2/3
        const int64_t kshift = 1 - (ir & 1);
        int64_t ip = (jp + jm - n + kshift + 1 + 2 * nl4) >> 1;
        ip %= nl4;
        return hp_ncap(res) + (ir - 1) * nl4 + ip;
    }
    const double tp = tt - floor(tt);
    const double tmp = za < 0.99 ? (double)n * sqrt(3.0 * (1.0 - za)) : (double)n * fabs(sin(theta)) / sqrt((1.0 + za) / 3.0);
    const int64_t jp = (int64_t)(tp * tmp), jm = (int64_t)((1.0 - tp) * tmp);
    int64_t ir = jp + jm + 1;  // the ring, counted from the nearer pole
    if (ir > n) ir = n;
    int64_t ip = (int64_t)(tt * (double)ir);
    if (ip > 4 * ir - 1) ip = 4 * ir - 1;
    return z > 0.0 ? 2 * ir * (ir - 1) + ip : hp_npix(res) - 2 * ir * (ir + 1) + ip;
}

// The cap predicate's left side, in the reference's form (layer.py:730-732) with thetac = pi / 2 - theta; sd, cd = sin, cos of the centre's
// declination.  A pixel belongs to the cap when this is >= cos(radius).
HP_HD double hp_cap_mu(double sd, double cd, double ra, double theta, double phi)
{
    HP_SEPARATE_ROUNDINGS
    const double thetac = HP_HALFPI - theta;
    const double a = sin(thetac) * sd, b = cos(thetac) * cd, c = ra - phi;
    const double bc = b * cos(c);
    return a + bc;
}

// The reference's pixel range (layer.py:721-725): pmin .. pmax, the pixels that hold (ra, dec +- (radius + 3 / nside)) with the declination
// clipped at the poles.
HP_HD void hp_cap_range(int res, double ra, double dec, double radius, int64_t *pmin, int64_t *pmax)
{
    HP_SEPARATE_ROUNDINGS
    const double radext = radius + 3.0 / (double)hp_nside(res);
    const double lo = dec - radext, hi = dec + radext;
    const double dmin = lo > -HP_HALFPI ? lo : -HP_HALFPI, dmax = hi < HP_HALFPI ? hi : HP_HALFPI;
    *pmin = hp_ang2pix(res, HP_HALFPI - dmax, ra);
    *pmax = hp_ang2pix(res, HP_HALFPI - dmin, ra);
}

// The part of a ring (colatitude theta, sine sth) that a cap of `radius` about (theta0, ra), ra in [0, 2 pi), can reach, one pixel wider on
// each side: *count pixels from index *first on, cyclically.  count = len: the whole ring (the cap reaches over it, or nearly).  count = 0:
// the ring lies outside.  From sin^2(dphi / 2) = sin((r + d) / 2) sin((r - d) / 2) / (sin theta sin theta0), d = theta - theta0, which is
// (cos r - z z0) / (sin theta sin theta0) = cos(dphi) without its cancellation.  The window only bounds the work: hp_cap_mu decides.
HP_HD void hp_ring_window(double theta, double sth, double theta0, double s0, double radius, double ra, const HpRing &g, int64_t *first, int64_t *count)
{
    const double d = theta - theta0, ad = fabs(d);
    *first = 0, *count = 0;
    if (ad > radius * (1.0 + 1e-12) + 1e-15) return;  // every point of the ring is at least |d| from the centre
    *count = g.len;
    const double den = sth * s0;
    const double h = radius > ad ? sin(0.5 * (radius + d)) * sin(0.5 * (radius - d)) : 0.0;
    if (!(den > 0.0) || !(h < den)) return;
    const double dphi = 2.0 * asin(sqrt(h / den)), step = HP_TWOPI / (double)g.len, off = g.shifted ? 0.5 : 0.0;
    const int64_t lo = (int64_t)floor((ra - dphi) / step - off) - 1, hi = (int64_t)ceil((ra + dphi) / step - off) + 1;
    if (hi - lo + 1 >= g.len) return;
    *count = hi - lo + 1;
    int64_t f = lo % g.len;
    *first = f < 0 ? f + g.len : f;
}

// Entry k of a window's traversal, ascending in the index: the segment that wrapped past phi = 0 comes first.
HP_HD int64_t hp_window_index(const HpRing &g, int64_t first, int64_t count, int64_t k)
{
    const int64_t nlow = first + count > g.len ? first + count - g.len : 0;
    return k < nlow ? k : first + (k - nlow);
}

// The box of analysis.py:967-973 for one coordinate: bdpad <= rint(v) < n - bdpad, and outside where rint(v) does not fit int16 or v is NaN.
HP_HD bool hp_in_box(double v, int n, int bdpad)
{
    const double r = rint(v);
    return r >= -32768.0 && r <= 32767.0 && r >= (double)bdpad && r < (double)(n - bdpad);
}

// The position angle of truthcats.py:240-241 from the two displaced positions, in degrees in [0, 360).
HP_HD double hp_position_angle(double xpp, double ypp, double xmm, double ymm)
{
    HP_SEPARATE_ROUNDINGS
    double pa = atan2(xpp - xmm, ypp - ymm) * 180.0 / HP_PI;
    const double turns = floor(pa / 360.0);
    pa -= 360.0 * turns;
    return pa >= 360.0 ? 0.0 : pa;
}

}  // namespace imcom
