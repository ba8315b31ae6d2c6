// starmom_core.h -- the arithmetic of starmom.hip that has one right answer and no device in it: the adaptive-moment iteration of a star
// (Bernstein & Jarvis 2002; Hirata & Seljak 2003; the iteration behind GalSim's FindAdaptiveMom, whose HSMParams defaults are the defaults of
// imcom_star_params): the state, the rows and columns of the weight ellipse rho2 <= nsig2, the step from the seven weighted sums to the next
// state with its exit decision, and the conversion to the result columns.  The sums themselves are the kernel's (and the check's) loops.
// Compiles as host code too (tests/native/starmom_check.cpp).
//
// The ranges decide which pixels are summed, so they are formed as the float64 restatement (tests/starcat_reference.py) forms them: every
// operation rounded once, in the written order.  Contraction is switched off in every function below.
#pragma once
#include <cmath>

#include "../../include/imcom_hip.h"

#ifdef __HIPCC__
#define SM_HD __host__ __device__ __forceinline__
#else
#define SM_HD inline
#endif

namespace imcom {

enum SmStatus {
    SM_OK = 0,
    SM_NOT_POSITIVE_DEFINITE = 1,  // detM, Mxx, Myy or semi_b2 not above zero
    SM_EMPTY_BOUNDS = 2,           // no row of the image inside the weight ellipse
    SM_TOO_LARGE = 3,              // a moment above max_amoment or a centroid shift above max_ashift
    SM_TOO_MANY_ITERATIONS = 4,
    SM_NAN = 5,                    // the convergence factor or the amplitude is NaN (an all-zero cut divides by A = 0)
    SM_RUNNING = -1
};

constexpr int SM_NSUMS = 7;  // A, Bx, By, Cxx, Cxy, Cyy, rho4
// The result columns of a star (imcom_star_moments writes SM_NCOL doubles a star).
enum SmCol {
    SMC_AMP = 0, SMC_X, SMC_Y, SMC_SIGMA, SMC_E1, SMC_E2, SMC_G1, SMC_G2, SMC_RHO4, SMC_NITER, SMC_STATUS, SMC_CF,
    SMC_SUM_WTI, SMC_SUM_M42RE, SMC_SUM_M42IM, SMC_SUM_WTI2, SMC_SUM_PLUS, SMC_SUM_CROSS,
    SMC_M42_REAL, SMC_M42_IMAG, SMC_FORCED_PLUS, SMC_FORCED_CROSS, SM_NCOL
};
constexpr int SM_MAX_SIDE = 127;
constexpr long SM_MAX_FRAME = 1L << 40;  // most elements (rows x pitch) of a frame

SM_HD double sm_sqrt(double v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(v);
#else
    return std::sqrt(v);
#endif
}
// std::max as C++ has it (the first argument if the comparison is false: a NaN in front stays)
SM_HD double sm_max(double a, double b) { return a < b ? b : a; }
SM_HD double sm_clip(double v, double bound)
{
    if (v > bound) v = bound;
    if (v < -bound) v = -bound;
    return v;
}

struct SmState {
    double x0, y0, Mxx, Mxy, Myy;        // the weight: centroid (1-based pixel coordinates) and moments
    double x00, y00, shiftscale0;        // the start centroid, the first iteration's shift scale
    double detM, Minv_xx, TwoMinv_xy, Minv_yy;  // of the running iteration (sm_begin)
    double cf;                           // the last convergence factor
    int iter;                            // completed iterations
    int status;                          // SM_RUNNING until the iteration ends
};

SM_HD void sm_init(SmState &s, int w, int h, const imcom_star_params &p)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    s.x0 = s.x00 = (1.0 + (double)w) / 2.0;
    s.y0 = s.y00 = (1.0 + (double)h) / 2.0;
    s.Mxx = s.Myy = p.guess_sig * p.guess_sig;
    s.Mxy = 0.0;
    s.shiftscale0 = 0.0;
    s.detM = s.Minv_xx = s.TwoMinv_xy = s.Minv_yy = 0.0;
    s.cf = 1.0;
    s.iter = 0;
    s.status = SM_RUNNING;
}

// The head of an iteration: the inverse of M and the rows iy1 .. iy2 (1-based, inclusive) the ellipse touches.  False: the state has failed.
SM_HD bool sm_begin(SmState &s, int h, const imcom_star_params &p, int *iy1, int *iy2)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double mxy2 = s.Mxy * s.Mxy;
    const double mxxyy = s.Mxx * s.Myy;
    s.detM = mxxyy - mxy2;
    if (!(s.detM > 0.0 && s.Mxx > 0.0 && s.Myy > 0.0)) {  // (a NaN fails too)
        s.status = SM_NOT_POSITIVE_DEFINITE;
        return false;
    }
    s.Minv_xx = s.Myy / s.detM;
    s.TwoMinv_xy = (-2.0 * s.Mxy) / s.detM;
    s.Minv_yy = s.Mxx / s.detM;
    const double y2 = sm_sqrt(p.max_moment_nsig2 * s.Myy);
    const double lo = sm_max(std::ceil(s.y0 - y2), 1.0), hi = std::fmin(std::floor(s.y0 + y2), (double)h);
    if (!(lo <= hi)) {
        s.status = SM_EMPTY_BOUNDS;
        return false;
    }
    *iy1 = (int)lo, *iy2 = (int)hi;
    return true;
}

// Row iy of the running iteration: dy, b, and the columns ix1 .. ix2 (1-based, inclusive).  False: the row holds no pixel of the ellipse.
SM_HD bool sm_row(const SmState &s, int iy, int w, const imcom_star_params &p, double *dy_, double *b_, int *ix1, int *ix2)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dy = (double)iy - s.y0;
    const double b = s.TwoMinv_xy * dy;
    const double q = s.Minv_yy * dy;
    const double qq = q * dy;
    const double c = qq - p.max_moment_nsig2;
    const double bb = b * b;
    const double a4 = 4.0 * s.Minv_xx;
    const double a4c = a4 * c;
    const double d = bb - a4c;
    *dy_ = dy, *b_ = b;
    if (!(d >= 0.0)) return false;
    const double sqrtd = sm_sqrt(d);
    const double inv2 = 0.5 / s.Minv_xx;
    const double t1 = -b - sqrtd;
    const double t2 = -b + sqrtd;
    const double p1 = inv2 * t1;
    const double p2 = inv2 * t2;
    const double x1 = s.x0 + p1;
    const double x2 = s.x0 + p2;
    const double lo = sm_max(std::ceil(x1), 1.0), hi = std::fmin(std::floor(x2), (double)w);
    if (!(lo <= hi)) return false;
    *ix1 = (int)lo, *ix2 = (int)hi;
    return true;
}

// One pixel of a row into the seven sums: column ix (1-based) with value `data`.
SM_HD void sm_pixel(const SmState &s, int ix, double dy, double b, double data, double *sum)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dx = (double)ix - s.x0;
    const double r1 = (s.Minv_yy * dy) * dy;
    const double r2 = b * dx;
    const double r3 = (s.Minv_xx * dx) * dx;
    const double rho2 = (r1 + r2) + r3;
    const double I = std::exp(-0.5 * rho2) * data;
    const double Ix = I * dx, Iy = I * dy;
    sum[0] += I;
    sum[1] += Ix;
    sum[2] += Iy;
    sum[3] += Ix * dx;
    sum[4] += Ix * dy;
    sum[5] += Iy * dy;
    sum[6] += (I * rho2) * rho2;
}

// The tail of an iteration: from the seven sums to the next state.  True: the iteration goes on; false: s.status says how it ended.
SM_HD bool sm_step(SmState &s, const double *sum, const imcom_star_params &p)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double A = sum[0], Bx = sum[1], By = sum[2], Cxx = sum[3], Cxy = sum[4], Cyy = sum[5];
    const double two_psi = std::atan2(2.0 * s.Mxy, s.Mxx - s.Myy);
    const double tr = s.Mxx + s.Myy;
    double semi_a2 = 0.5 * (tr + (s.Mxx - s.Myy) * std::cos(two_psi)) + s.Mxy * std::sin(two_psi);
    const double semi_b2 = tr - semi_a2;
    if (!(semi_b2 > 0.0)) {
        s.status = SM_NOT_POSITIVE_DEFINITE;
        return false;
    }
    const double shiftscale = sm_sqrt(semi_b2);
    if (s.iter == 0) s.shiftscale0 = shiftscale;
    double dx = 2.0 * Bx / (A * shiftscale);
    double dy = 2.0 * By / (A * shiftscale);
    double dxx = 4.0 * (Cxx / A - 0.5 * s.Mxx) / semi_b2;
    double dxy = 4.0 * (Cxy / A - 0.5 * s.Mxy) / semi_b2;
    double dyy = 4.0 * (Cyy / A - 0.5 * s.Myy) / semi_b2;
    dx = sm_clip(dx, p.bound_correct_wt);
    dy = sm_clip(dy, p.bound_correct_wt);
    dxx = sm_clip(dxx, p.bound_correct_wt);
    dxy = sm_clip(dxy, p.bound_correct_wt);
    dyy = sm_clip(dyy, p.bound_correct_wt);
    double cf = sm_max(std::fabs(dx), std::fabs(dy));
    cf = cf * cf;
    cf = sm_max(cf, std::fabs(dxx));
    cf = sm_max(cf, std::fabs(dxy));
    cf = sm_max(cf, std::fabs(dyy));
    cf = sm_sqrt(cf);
    if (shiftscale < s.shiftscale0) cf *= s.shiftscale0 / shiftscale;
    s.x0 += dx * shiftscale;
    s.y0 += dy * shiftscale;
    s.Mxx += dxx * semi_b2;
    s.Mxy += dxy * semi_b2;
    s.Myy += dyy * semi_b2;
    s.cf = cf;
    s.iter++;
    if (std::fabs(s.Mxx) > p.max_amoment || std::fabs(s.Mxy) > p.max_amoment || std::fabs(s.Myy) > p.max_amoment || std::fabs(s.x0 - s.x00) > p.max_ashift ||
        std::fabs(s.y0 - s.y00) > p.max_ashift) {
        s.status = SM_TOO_LARGE;
        return false;
    }
    if (s.iter > p.max_mom2_iter) {
        s.status = SM_TOO_MANY_ITERATIONS;
        return false;
    }
    if (cf != cf || A != A) {
        s.status = SM_NAN;
        return false;
    }
    if (!(cf > p.convergence_threshold)) {
        s.status = SM_OK;
        return false;
    }
    return true;
}

// The result columns of a converged state (its moments as the last step left them); `sum` the sums of its last iteration.
SM_HD void sm_finish(const SmState &s, const double *sum, double *col)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double A = sum[0];
    col[SMC_AMP] = 2.0 * A;
    col[SMC_X] = s.x0;
    col[SMC_Y] = s.y0;
    const double det = s.Mxx * s.Myy - s.Mxy * s.Mxy;
    col[SMC_SIGMA] = sm_sqrt(sm_sqrt(det));
    const double tr = s.Mxx + s.Myy;
    const double e1 = (s.Mxx - s.Myy) / tr, e2 = 2.0 * s.Mxy / tr;
    const double esq = e1 * e1 + e2 * e2;
    const double g = 1.0 / (1.0 + sm_sqrt(1.0 - esq));
    col[SMC_E1] = e1, col[SMC_E2] = e2;
    col[SMC_G1] = e1 * g, col[SMC_G2] = e2 * g;
    col[SMC_RHO4] = sum[6] / A;
}

// What the higher-moment pass of analysis.py:1021-1027 needs of a result: u_ = (cu_x x_ - Mxy y_) / rz, v_ = (cv_y y_ - Mxy x_) / rz.
struct SmHigher {
    double cu_x, cv_y, Mxy, rz;
};
SM_HD SmHigher sm_higher(const double *col)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double sigma = col[SMC_SIGMA], e1 = col[SMC_E1], e2 = col[SMC_E2];
    const double s2 = sigma * sigma;
    const double root = sm_sqrt(1.0 - e1 * e1 - e2 * e2);
    const double Mxx = s2 * (1.0 + e1) / root;
    const double Myy = s2 * (1.0 - e1) / root;
    const double Mxy = s2 * e2 / root;
    const double D = Mxx * Myy - Mxy * Mxy;
    const double rD = sm_sqrt(D);
    const double zeta = D * (Mxx + Myy + 2.0 * rD);
    SmHigher k;
    k.cu_x = Myy + rD;
    k.cv_y = Mxx + rD;
    k.Mxy = Mxy;
    k.rz = sm_sqrt(zeta);
    return k;
}

// One pixel of the two passes 1016-1041: x_, y_ its offsets from the centroid, `data` its value; sums 0-2: wti, wti (u^4 - v^4),
// wti (u^3 v + u v^3); with a forced scale (fs2 = forced_scale^2 > 0) sums 3-5: wti2, wti2 (x^2 - y^2), wti2 (2 x y).
SM_HD void sm_higher_pixel(const SmHigher &k, double x_, double y_, double data, double fs2, double *sum)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double u = (k.cu_x * x_ - k.Mxy * y_) / k.rz;
    const double v = (k.cv_y * y_ - k.Mxy * x_) / k.rz;
    const double u2 = u * u, v2 = v * v;
    const double wti = data * std::exp(-0.5 * (u2 + v2));
    sum[0] += wti;
    sum[1] += wti * (u2 * u2 - v2 * v2);
    sum[2] += wti * (u2 * u * v + u * (v2 * v));
    if (fs2 > 0.0) {
        const double x2 = x_ * x_, y2 = y_ * y_;
        const double wti2 = data * std::exp(-0.5 * (x2 + y2) / fs2);
        sum[3] += wti2;
        sum[4] += wti2 * (x2 - y2);
        sum[5] += wti2 * (2.0 * x_ * y_);
    }
}

SM_HD void sm_higher_finish(const double *sum, double fs2, double *col)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    col[SMC_SUM_WTI] = sum[0], col[SMC_SUM_M42RE] = sum[1], col[SMC_SUM_M42IM] = sum[2];
    col[SMC_SUM_WTI2] = sum[3], col[SMC_SUM_PLUS] = sum[4], col[SMC_SUM_CROSS] = sum[5];
    col[SMC_M42_REAL] = sum[1] / sum[0];
    col[SMC_M42_IMAG] = 2.0 * sum[2] / sum[0];
    if (fs2 > 0.0) {
        col[SMC_FORCED_PLUS] = sum[4] / sum[3] / fs2;
        col[SMC_FORCED_CROSS] = sum[5] / sum[3] / fs2;
    }
}

}  // namespace imcom
