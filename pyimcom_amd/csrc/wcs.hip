// wcs.hip -- world coordinate systems on the device: the closed arithmetic that the reference's PyIMCOM_WCS reduces a WCS to
// (src/pyimcom/wcsutil.py:419-634: a FITS TAN-SIP header, or for gwcs input a fitted TAN-SIP plus a bilinear error map), the pixel ->
// pixel map of compareutils.map_sca2sca (src/pyimcom/utils/compareutils.py:63-106) and the pixel areas of wcsutil.get_pix_area
// (wcsutil.py:688-788).  The per-point arithmetic is wcs_core.h's.
//
// One thread owns a point (WCS_ITEMS points, a workgroup's tile apart, so that a wave's store is contiguous).  The descriptors travel as
// kernel arguments, so every coefficient is wave-uniform; the only gathers are the eight taps of an error-table look-up (four in each of its two
// planes).
// Counts are summed as integers inside a workgroup and added once a workgroup; there is no float atomic and no float sum across threads, so
// the results are the same bits for every run and every chunking.  The C entries imcom_wcs_* end destripe.hip, the first consumer's file.
#include <algorithm>

#include "launchers.h"
#include "wcs_core.h"

namespace imcom {

namespace {

constexpr int WCS_THREADS = 256, WCS_ITEMS = 4, WCS_TILE = WCS_THREADS * WCS_ITEMS;

struct WcsMat {
    double m[9];
};

struct WcsGrid {  // point k of a grid: (x, y) = (lox + (k % nx) stepx, loy + (k / nx) stepy)
    double lox, stepx, loy, stepy;
    int nx, ny;
};

// The sum of a and of b over the workgroup, added to out[0] and out[1] by one thread (integers: the order does not matter).
__device__ __forceinline__ void wcs_block_counts(unsigned a, unsigned b, unsigned long long *out)
{
    __shared__ unsigned lds[2][WCS_THREADS / 64];
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_down(a, d, 64);
        b += __shfl_down(b, d, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) lds[0][w] = a, lds[1][w] = b;
    __syncthreads();
    if (threadIdx.x == 0 && out) {
        unsigned sa = 0, sb = 0;
        for (int k = 0; k < WCS_THREADS / 64; k++) sa += lds[0][k], sb += lds[1][k];
        if (sa) atomicAdd(out, (unsigned long long)sa);
        if (sb) atomicAdd(out + 1, (unsigned long long)sb);
    }
}

// in [n][2] -> out [n][2]: pixel -> (ra, dec) in degrees, or (inverse) (ra, dec) -> pixel.  bad[1] counts the points written NaN.
__global__ __launch_bounds__(WCS_THREADS) void wcs_list_kernel(const WcsDesc w, const WcsTab t, int inverse, const double2 *__restrict__ in, long n, int origin,
                                                              double2 *__restrict__ out, unsigned long long *bad)
{
    unsigned nbad = 0;
    const long p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long p = p0 + (long)i * WCS_THREADS;
        if (p >= n) break;
        const double2 q = in[p];
        double2 r;
        if (inverse) wcs_world2pix(w, t, q.x, q.y, origin, &r.x, &r.y);
        else wcs_pix2world(w, t, q.x, q.y, origin, &r.x, &r.y);
        if (!(r.x - r.x == 0.0 && r.y - r.y == 0.0)) {
            r.x = NAN, r.y = NAN;
            nbad++;
        }
        out[p] = r;
    }
    wcs_block_counts(0u, nbad, bad);
}

// Points of `from` (a list pts [n][2], or the grid g) -> pixels of `to`: xo, yo [n] float64 or float32 (either may be null), mask [n] the
// is_in_ref of compareutils.py:103-105 from the float64 positions (may be null), counts[0] += points in the reference, counts[1] += points
// written NaN.
__global__ __launch_bounds__(WCS_THREADS) void wcs_pix2pix_kernel(const WcsDesc from, const WcsTab tf, const WcsDesc to, const WcsTab tt, const WcsMat M,
                                                                 const double2 *__restrict__ pts, const WcsGrid g, long n, int origin, double nside, double pad,
                                                                 void *__restrict__ xo, void *__restrict__ yo, int f32, unsigned char *__restrict__ mask,
                                                                 unsigned long long *counts)
{
    unsigned nin = 0, nbad = 0;
    const long p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long p = p0 + (long)i * WCS_THREADS;
        if (p >= n) break;
        double x, y;
        if (pts) {
            const double2 q = pts[p];
            x = q.x, y = q.y;
        } else {
            const long iy = p / g.nx;
            x = g.lox + (double)(p - iy * g.nx) * g.stepx;
            y = g.loy + (double)iy * g.stepy;
        }
        double xf, yf;
        if (!wcs_pix2pix(from, tf, to, tt, M.m, x, y, origin, &xf, &yf) || !(xf - xf == 0.0 && yf - yf == 0.0)) {
            xf = NAN, yf = NAN;
            nbad++;
        }
        const bool in = wcs_is_in_ref(xf, yf, nside, pad);
        nin += in ? 1u : 0u;
        if (f32) {
            if (xo) ((float *)xo)[p] = (float)xf;
            if (yo) ((float *)yo)[p] = (float)yf;
        } else {
            if (xo) ((double *)xo)[p] = xf;
            if (yo) ((double *)yo)[p] = yf;
        }
        if (mask) mask[p] = in ? 1 : 0;
    }
    wcs_block_counts(nin, nbad, counts);
}

// A double as an unsigned integer of the same order (NaN aside).
__device__ __forceinline__ unsigned long long wcs_order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// get_pix_area, first launch (wcsutil.py:729-734): ra, dec [H][W] in degrees of the pixels (xs[i], ys[j]), and ext = {key of min ra, key of
// max ra} over the frame (integer atomics on order keys: exact, whatever the order).
__global__ __launch_bounds__(WCS_THREADS) void wcs_area_frame_kernel(const WcsDesc w, const WcsTab t, const double *__restrict__ xs, int W, const double *__restrict__ ys,
                                                                    int H, double *__restrict__ ra, double *__restrict__ dec, unsigned long long *ext)
{
    __shared__ unsigned long long lds[2][WCS_THREADS / 64];
    const long n = (long)W * H, p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
    unsigned long long lo = ~0ull, hi = 0ull;
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long p = p0 + (long)i * WCS_THREADS;
        if (p >= n) break;
        const long j = p / W;
        double a, d;
        wcs_pix2world(w, t, xs[p - j * W], ys[j], 0, &a, &d);
        ra[p] = a, dec[p] = d;
        if (a == a) {
            const unsigned long long k = wcs_order_key(a);
            lo = k < lo ? k : lo, hi = k > hi ? k : hi;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long l2 = __shfl_down(lo, d, 64), h2 = __shfl_down(hi, d, 64);
        lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) lds[0][threadIdx.x >> 6] = lo, lds[1][threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < WCS_THREADS / 64; k++) {
            lo = lds[0][k] < lo ? lds[0][k] : lo;
            hi = lds[1][k] > hi ? lds[1][k] : hi;
        }
        atomicMin(ext, lo);
        atomicMax(ext + 1, hi);
    }
}

// The footprint turned away from the prime meridian (wcsutil.py:740-749): (ra, dec) in the frame whose pole is the old y axis and whose
// ra = 180 is the old x axis.
__device__ __forceinline__ void wcs_area_turn(int rotate, double &a, double &d)
{
    if (!rotate) return;
    double c[3];
    wcs_world2vec(a, d, c);
    d = asin(c[1]) / WCS_DEG;
    a = atan2(-c[2], c[0]) / WCS_DEG + 180.0;
}

// get_pix_area, second launch (751-786): area [h][w] with h = H - 2 op, w = W - 2 op, op = ovsamp * pad; the centred differences of ra and
// dec in degrees, the determinant, cos(dec).
__global__ __launch_bounds__(WCS_THREADS) void wcs_area_finish_kernel(const double *__restrict__ ra, const double *__restrict__ dec, int W, int H, int op, double pad,
                                                                     int rotate, double *__restrict__ area)
{
    const int w = W - 2 * op, h = H - 2 * op;
    const long n = (long)w * h, p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long p = p0 + (long)i * WCS_THREADS;
        if (p >= n) break;
        const long j = p / w, c = p - j * w;
        const long at[5] = {(j + op) * W + c + 2 * op, (j + op) * W + c, (j + 2 * op) * W + c + op, j * W + c + op, (j + op) * W + c + op};
        double a[5], d[5];
        for (int k = 0; k < 5; k++) {
            a[k] = ra[at[k]], d[k] = dec[at[k]];
            wcs_area_turn(rotate, a[k], d[k]);
        }
        const double rx = (a[0] - a[1]) / 2.0 / pad, ry = (a[2] - a[3]) / 2.0 / pad, dx = (d[0] - d[1]) / 2.0 / pad, dy = (d[2] - d[3]) / 2.0 / pad;
        area[p] = fabs(rx * dy - ry * dx) * cos(d[4] * WCS_DEG);
    }
}

unsigned wcs_blocks(long n) { return (unsigned)std::max(1L, (n + WCS_TILE - 1) / WCS_TILE); }

}  // namespace

int launch_wcs_list(imcom_ctx *ctx, const WcsDesc &w, const WcsTab &t, int inverse, const double *in, long n, int origin, double *out, unsigned long long *counts)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_list_kernel, dim3(wcs_blocks(n)), dim3(WCS_THREADS), 0, ctx->stream, w, t, inverse, (const double2 *)in, n, origin, (double2 *)out, counts);
    return check_launch("wcs_list_kernel");
}

int launch_wcs_pix2pix(imcom_ctx *ctx, const WcsDesc &from, const WcsTab &tf, const WcsDesc &to, const WcsTab &tt, const double *M, const double *pts, const double *grid,
                       long n, int origin, double nside, double pad, void *xo, void *yo, int f32, unsigned char *mask, unsigned long long *counts)
{
    ProfScope ps(ctx, "wcs");
    WcsMat m;
    for (int k = 0; k < 9; k++) m.m[k] = M[k];
    WcsGrid g = {0, 0, 0, 0, 1, 1};
    if (grid) g = {grid[0], grid[1], grid[3], grid[4], (int)grid[2], (int)grid[5]};
    hipLaunchKernelGGL(wcs_pix2pix_kernel, dim3(wcs_blocks(n)), dim3(WCS_THREADS), 0, ctx->stream, from, tf, to, tt, m, (const double2 *)pts, g, n, origin, nside, pad, xo,
                       yo, f32, mask, counts);
    return check_launch("wcs_pix2pix_kernel");
}

int launch_wcs_area_frame(imcom_ctx *ctx, const WcsDesc &w, const WcsTab &t, const double *xs, int W, const double *ys, int H, double *ra, double *dec,
                          unsigned long long *ext)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_area_frame_kernel, dim3(wcs_blocks((long)W * H)), dim3(WCS_THREADS), 0, ctx->stream, w, t, xs, W, ys, H, ra, dec, ext);
    return check_launch("wcs_area_frame_kernel");
}

int launch_wcs_area_finish(imcom_ctx *ctx, const double *ra, const double *dec, int W, int H, int op, double pad, int rotate, double *area)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_area_finish_kernel, dim3(wcs_blocks((long)(W - 2 * op) * (H - 2 * op))), dim3(WCS_THREADS), 0, ctx->stream, ra, dec, W, H, op, pad, rotate,
                       area);
    return check_launch("wcs_area_finish_kernel");
}

double wcs_key_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, 8);
    return v;
}

}  // namespace imcom
