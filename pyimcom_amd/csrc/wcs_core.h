// wcs_core.h -- the per-point arithmetic of wcs.hip: a FITS world coordinate system reduced to closed arithmetic (FITS WCS papers I / II,
// Greisen & Calabretta 2002, Calabretta & Greisen 2002; the SIP convention, Shupe et al. 2005), as the reference's PyIMCOM_WCS uses it
// (src/pyimcom/wcsutil.py:419-634): pixel -> SIP polynomial -> CD matrix -> zenithal projection (TAN or STG) -> rotation of the sphere, the
// inverse of each, and the bilinear error map of the "ASTROPY+" type (LocWCS.err_interp, wcsutil.py:364-413).  One point has one owner and
// nothing is reduced.  Compiles as host code too (tests/native/wcs_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define WCS_HD __host__ __device__ __forceinline__
#else
#define WCS_HD inline
#endif

namespace imcom {

// The descriptor of one WCS: WCS_DESC_LEN doubles, packed by the caller (include/imcom_hip.h states the same layout).
//   [0] projection (0 TAN, 1 STG)   [1] CRPIX1  [2] CRPIX2   [3..6] CD1_1 CD1_2 CD2_1 CD2_2 (degrees a pixel)
//   [7..15] the rotation R, row-major: native unit vector = R (celestial unit vector) (Paper II eq. 2 with the native pole at CRVAL)
//   [16] A_ORDER  [17] B_ORDER (0: none; up to WCS_MAX_ORDER)   [18] niter (error map only)   [19] reserved, 0
//   [20 .. 74] A_p_q   [75 .. 129] B_p_q, each at wcs_sip_index(p, q), p + q <= 9; the entries above the order are not read
constexpr int WCS_MAX_ORDER = 9;
constexpr int WCS_SIP_COEFFS = (WCS_MAX_ORDER + 1) * (WCS_MAX_ORDER + 2) / 2;  // 55
constexpr int WCS_D_PROJ = 0, WCS_D_CRPIX = 1, WCS_D_CD = 3, WCS_D_ROT = 7, WCS_D_AORDER = 16, WCS_D_BORDER = 17, WCS_D_NITER = 18, WCS_D_A = 20,
              WCS_D_B = WCS_D_A + WCS_SIP_COEFFS, WCS_DESC_LEN = WCS_D_B + WCS_SIP_COEFFS;  // 130
constexpr int WCS_TAN = 0, WCS_STG = 1;
constexpr int WCS_NEWTON_CAP = 12;
constexpr int WCS_MAX_NITER = 16;
constexpr double WCS_NEWTON_TOL = 9.094947017729282e-13;  // 2^-40 pixel
constexpr double WCS_NEWTON_REL = 2.220446049250313e-16;  // 2^-52 of the coordinate (between one and two ulps)
constexpr double WCS_DEG = 0.017453292519943295;           // pi / 180
constexpr double WCS_RAD = 57.29577951308232;              // 180 / pi

struct WcsDesc {
    double d[WCS_DESC_LEN];
};

// The padded error table of one WCS (device memory, or host memory in the native check): values [2][n2][n2], plane 0 the x offset and
// plane 1 the y offset, axes (y, x); n2 = N + 2 nodes an axis at lo, 0, 1, .., N - 1, hi.  p == nullptr: no table.
struct WcsTab {
    const void *p;
    int f64, n2;
    double lo, hi;
};

WCS_HD int wcs_sip_index(int p, int q) { return p * (WCS_MAX_ORDER + 1) - p * (p - 1) / 2 + q; }

// f = sum_{p + q <= order} c_pq u^p v^q and its two derivatives, by Horner in v inside Horner in u.
WCS_HD void wcs_sip_eval(const double *c, int order, double u, double v, double *f, double *fu, double *fv)
{
    double F = 0.0, Fu = 0.0, Fv = 0.0;
    for (int p = order; p >= 0; p--) {
        const double *row = c + wcs_sip_index(p, 0);
        double g = 0.0, gv = 0.0;
        for (int q = order - p; q >= 0; q--) {
            gv = gv * v + g;
            g = g * v + row[q];
        }
        Fu = Fu * u + F;
        F = F * u + g;
        Fv = Fv * u + gv;
    }
    *f = F, *fu = Fu, *fv = Fv;
}

// Pixel -> intermediate world coordinates (xi, eta) in radians.
WCS_HD void wcs_pix2inter(const WcsDesc &w, double x, double y, int origin, double *xi, double *eta)
{
    const double u = x + (double)(1 - origin) - w.d[WCS_D_CRPIX], v = y + (double)(1 - origin) - w.d[WCS_D_CRPIX + 1];
    double up = u, vp = v, f, fu, fv;
    const int ao = (int)w.d[WCS_D_AORDER], bo = (int)w.d[WCS_D_BORDER];
    if (ao > 0) {
        wcs_sip_eval(w.d + WCS_D_A, ao, u, v, &f, &fu, &fv);
        up = u + f;
    }
    if (bo > 0) {
        wcs_sip_eval(w.d + WCS_D_B, bo, u, v, &f, &fu, &fv);
        vp = v + f;
    }
    *xi = (w.d[WCS_D_CD] * up + w.d[WCS_D_CD + 1] * vp) * WCS_DEG;
    *eta = (w.d[WCS_D_CD + 2] * up + w.d[WCS_D_CD + 3] * vp) * WCS_DEG;
}

// Intermediate -> native unit vector (cos theta cos phi, cos theta sin phi, sin theta), phi = atan2(xi, -eta); no trigonometry.
WCS_HD void wcs_inter2native(int proj, double xi, double eta, double n[3])
{
    const double r2 = xi * xi + eta * eta;
    if (proj == WCS_TAN) {
        const double s = 1.0 / sqrt(1.0 + r2);
        n[0] = -eta * s, n[1] = xi * s, n[2] = s;
    } else {
        const double s = 1.0 / (4.0 + r2);
        n[0] = -4.0 * eta * s, n[1] = 4.0 * xi * s, n[2] = (4.0 - r2) * s;
    }
}

// c = R^T n (native -> celestial) and n = R c (celestial -> native); M of wcs_apply is any row-major 3 x 3.
WCS_HD void wcs_apply_t(const double *R, const double n[3], double c[3])
{
    c[0] = R[0] * n[0] + R[3] * n[1] + R[6] * n[2];
    c[1] = R[1] * n[0] + R[4] * n[1] + R[7] * n[2];
    c[2] = R[2] * n[0] + R[5] * n[1] + R[8] * n[2];
}
WCS_HD void wcs_apply(const double *M, const double c[3], double n[3])
{
    n[0] = M[0] * c[0] + M[1] * c[1] + M[2] * c[2];
    n[1] = M[3] * c[0] + M[4] * c[1] + M[5] * c[2];
    n[2] = M[6] * c[0] + M[7] * c[1] + M[8] * c[2];
}

// Celestial unit vector <-> (ra, dec) in degrees, ra in [0, 360).
WCS_HD void wcs_vec2world(const double c[3], double *ra, double *dec)
{
    double a = atan2(c[1], c[0]) * WCS_RAD;
    if (a < 0.0) a += 360.0;
    if (a >= 360.0) a = 0.0;  // (-tiny + 360 rounds to 360)
    *ra = a;
    *dec = atan2(c[2], hypot(c[0], c[1])) * WCS_RAD;
}
WCS_HD void wcs_world2vec(double ra, double dec, double c[3])
{
    const double a = ra * WCS_DEG, d = dec * WCS_DEG, cd = cos(d);
    c[0] = cd * cos(a), c[1] = cd * sin(a), c[2] = sin(d);
}

// Native unit vector -> pixel: the projection, CD^-1 in closed form, the SIP by Newton from the linear solution with the analytic
// Jacobian (at most WCS_NEWTON_CAP steps, until both components of a step are below 2^-40 pixel, or below 2^-52 of the coordinate where that
// is more: far off the chip 2^-40 pixel is less than an ulp).  false, and NaN in both outputs: the far
// hemisphere of TAN (n_z <= 0), the antipode of STG, input that is not finite, or an iteration that has not stopped.
WCS_HD bool wcs_native2pix(const WcsDesc &w, const double n[3], int origin, double *x, double *y)
{
    const double nan = NAN;
    *x = nan, *y = nan;
    const int proj = (int)w.d[WCS_D_PROJ];
    double xi, eta;
    if (!(n[0] - n[0] == 0.0 && n[1] - n[1] == 0.0 && n[2] - n[2] == 0.0)) return false;
    if (proj == WCS_TAN) {
        if (!(n[2] > 0.0)) return false;
        xi = n[1] / n[2], eta = -n[0] / n[2];
    } else {
        const double s = 1.0 + n[2];
        if (!(s > 0.0)) return false;
        xi = 2.0 * n[1] / s, eta = -2.0 * n[0] / s;
    }
    if (!(xi - xi == 0.0 && eta - eta == 0.0)) return false;  // (an overflow next to the antipode)
    xi *= WCS_RAD, eta *= WCS_RAD;
    const double c11 = w.d[WCS_D_CD], c12 = w.d[WCS_D_CD + 1], c21 = w.d[WCS_D_CD + 2], c22 = w.d[WCS_D_CD + 3];
    const double det = c11 * c22 - c12 * c21;
    const double U = (c22 * xi - c12 * eta) / det, V = (c11 * eta - c21 * xi) / det;
    double u = U, v = V;
    const int ao = (int)w.d[WCS_D_AORDER], bo = (int)w.d[WCS_D_BORDER];
    if (ao > 0 || bo > 0) {
        bool stopped = false;
        for (int it = 0; it < WCS_NEWTON_CAP && !stopped; it++) {
            double a = 0.0, au = 0.0, av = 0.0, b = 0.0, bu = 0.0, bv = 0.0;
            if (ao > 0) wcs_sip_eval(w.d + WCS_D_A, ao, u, v, &a, &au, &av);
            if (bo > 0) wcs_sip_eval(w.d + WCS_D_B, bo, u, v, &b, &bu, &bv);
            const double f1 = (u - U) + a, f2 = (v - V) + b;  // (the differences are exact or nearly so: the residual keeps the accuracy of a, b)
            const double j11 = 1.0 + au, j22 = 1.0 + bv, jd = j11 * j22 - av * bu;
            const double du = (j22 * f1 - av * f2) / jd, dv = (j11 * f2 - bu * f1) / jd;
            u -= du, v -= dv;
            // (false for NaN.)  More than 4096 pixels from CRPIX an ulp of the coordinate exceeds 2^-40 pixel and a step can alternate between
            // the two neighbours of the root for ever: there a step below 2^-52 of the coordinate has arrived
            stopped = fabs(du) < fmax(WCS_NEWTON_TOL, WCS_NEWTON_REL * fabs(u)) && fabs(dv) < fmax(WCS_NEWTON_TOL, WCS_NEWTON_REL * fabs(v));
        }
        if (!stopped) return false;
    }
    *x = u + w.d[WCS_D_CRPIX] - (double)(1 - origin);
    *y = v + w.d[WCS_D_CRPIX + 1] - (double)(1 - origin);
    return true;
}

// ---- the error map ----------------------------------------------------------------------------------------------------------------------

// The cell of coordinate t on the axis lo, 0, 1, .., N - 1, hi (n2 = N + 2 nodes): the i in 0 .. N with node[i] <= t < node[i + 1], the
// end cells for everything beyond (linear extrapolation), and the normalised distance (t - node[i]) / (node[i + 1] - node[i]).
WCS_HD double wcs_tab_node(int i, int n2, double lo, double hi) { return i == 0 ? lo : (i == n2 - 1 ? hi : (double)(i - 1)); }
WCS_HD int wcs_tab_cell(double t, int n2, double lo, double hi, double *frac)
{
    const int N = n2 - 2;
    int i;
    if (t < 0.0) i = 0;
    else if (t >= (double)(N - 1)) i = N;
    else i = 1 + (int)t;  // 0 <= t < N - 1
    const double a = wcs_tab_node(i, n2, lo, hi), b = wcs_tab_node(i + 1, n2, lo, hi);
    *frac = (t - a) / (b - a);
    return i;
}

template <typename T>
WCS_HD double wcs_tab_bilinear(const T *plane, int n2, int iy, int ix, double fy, double fx)
{
    const T *r0 = plane + (long)iy * n2 + ix, *r1 = r0 + n2;
    // the term order of scipy's linear evaluator on a 2-D grid: (0, 0), (0, 1), (1, 0), (1, 1), first axis y
    double s = (double)r0[0] * ((1.0 - fy) * (1.0 - fx));
    s += (double)r0[1] * ((1.0 - fy) * fx);
    s += (double)r1[0] * (fy * (1.0 - fx));
    s += (double)r1[1] * (fy * fx);
    return s;
}

// (dx, dy) of the point (x, y): each point's own correction, table axes (y, x).  A coordinate that is not finite gives NaN.
WCS_HD void wcs_tab_offsets(const WcsTab &t, double x, double y, double *dx, double *dy)
{
    if (!(x - x == 0.0 && y - y == 0.0)) {
        *dx = NAN, *dy = NAN;
        return;
    }
    double fx, fy;
    const int ix = wcs_tab_cell(x, t.n2, t.lo, t.hi, &fx), iy = wcs_tab_cell(y, t.n2, t.lo, t.hi, &fy);
    const long plane = (long)t.n2 * t.n2;
    if (t.f64) {
        *dx = wcs_tab_bilinear((const double *)t.p, t.n2, iy, ix, fy, fx);
        *dy = wcs_tab_bilinear((const double *)t.p + plane, t.n2, iy, ix, fy, fx);
    } else {
        *dx = wcs_tab_bilinear((const float *)t.p, t.n2, iy, ix, fy, fx);
        *dy = wcs_tab_bilinear((const float *)t.p + plane, t.n2, iy, ix, fy, fx);
    }
}

// ---- the chains -------------------------------------------------------------------------------------------------------------------------

// Pixel -> celestial unit vector (wcsutil.py:515-517 with a table: world(pos + dp(pos))).
WCS_HD void wcs_pix2vec(const WcsDesc &w, const WcsTab &t, double x, double y, int origin, double c[3])
{
    if (t.p) {
        double dx, dy;
        wcs_tab_offsets(t, x, y, &dx, &dy);
        x += dx, y += dy;
    }
    double xi, eta, n[3];
    wcs_pix2inter(w, x, y, origin, &xi, &eta);
    wcs_inter2native(w.d[WCS_D_PROJ] == 0.0 ? WCS_TAN : WCS_STG, xi, eta, n);
    wcs_apply_t(w.d + WCS_D_ROT, n, c);
}

// Native unit vector -> pixel (wcsutil.py:583-591 with a table: pos2 = inverse, then niter times pos1 = pos2 - dp(pos1) from pos1 = pos2).
WCS_HD bool wcs_native2pix_tab(const WcsDesc &w, const WcsTab &t, const double n[3], int origin, double *x, double *y)
{
    double x2, y2;
    const bool ok = wcs_native2pix(w, n, origin, &x2, &y2);
    double x1 = x2, y1 = y2;
    if (ok && t.p) {
        const int niter = (int)w.d[WCS_D_NITER];
        for (int k = 0; k < niter; k++) {
            double dx, dy;
            wcs_tab_offsets(t, x1, y1, &dx, &dy);
            x1 = x2 - dx, y1 = y2 - dy;
        }
    }
    *x = x1, *y = y1;
    return ok;
}

WCS_HD void wcs_pix2world(const WcsDesc &w, const WcsTab &t, double x, double y, int origin, double *ra, double *dec)
{
    double c[3];
    wcs_pix2vec(w, t, x, y, origin, c);
    wcs_vec2world(c, ra, dec);
}

WCS_HD bool wcs_world2pix(const WcsDesc &w, const WcsTab &t, double ra, double dec, int origin, double *x, double *y)
{
    double c[3], n[3];
    wcs_world2vec(ra, dec, c);
    wcs_apply(w.d + WCS_D_ROT, c, n);
    return wcs_native2pix_tab(w, t, n, origin, x, y);
}

// pixel of `from` -> pixel of `to` through the unit vector only; M = R_to R_from^T (row-major), formed by the host.
WCS_HD bool wcs_pix2pix(const WcsDesc &from, const WcsTab &tf, const WcsDesc &to, const WcsTab &tt, const double *M, double x, double y, int origin, double *xo,
                        double *yo)
{
    if (tf.p) {
        double dx, dy;
        wcs_tab_offsets(tf, x, y, &dx, &dy);
        x += dx, y += dy;
    }
    double xi, eta, nf[3], nt[3];
    wcs_pix2inter(from, x, y, origin, &xi, &eta);
    wcs_inter2native(from.d[WCS_D_PROJ] == 0.0 ? WCS_TAN : WCS_STG, xi, eta, nf);
    wcs_apply(M, nf, nt);
    return wcs_native2pix_tab(to, tt, nt, origin, xo, yo);
}

// compareutils.py:103-105: strict in x, not strict in y; formed from the float64 positions.  NaN is outside.
WCS_HD bool wcs_is_in_ref(double xf, double yf, double nside, double pad)
{
    return (xf + 0.5 + pad) * (nside - 0.5 - xf + pad) > 0.0 && (yf + 0.5 + pad) * (nside - 0.5 - yf + pad) >= 0.0;
}

}  // namespace imcom
