// wcs.hip -- world coordinate systems on the device: the closed arithmetic that the reference's PyIMCOM_WCS reduces a WCS to
// (src/pyimcom/wcsutil.py:419-634: a FITS TAN-SIP header, or for gwcs input a fitted TAN-SIP plus a bilinear error map), the pixel ->
// pixel map of compareutils.map_sca2sca (src/pyimcom/utils/compareutils.py:63-106) and the pixel areas of wcsutil.get_pix_area
// (wcsutil.py:688-788).  The per-point arithmetic is wcs_core.h's.
//
// One thread owns a point (WCS_ITEMS points, a workgroup's tile apart, so that a wave's store is contiguous).  The descriptors travel as
// kernel arguments, so every coefficient is wave-uniform; the only gathers are the eight taps of an error-table look-up (four in each of its two
// planes).
// Counts are summed as integers inside a workgroup and added once a workgroup; there is no float atomic and no float sum across threads, so
// the results are the same bits for every run and every chunking.  The C entries imcom_wcs_* end the file.
#include <algorithm>

#include "launchers.h"
#include "wcs_core.h"

namespace imcom {

namespace {

constexpr int WCS_THREADS = 256, WCS_ITEMS = 4, WCS_TILE = WCS_THREADS * WCS_ITEMS;
constexpr long WCS_MAX_POINTS = 1L << 40;  // most points of one call (the workgroups of 1024 points fit the launch's unsigned count)

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

static int launch_wcs_list(imcom_ctx *ctx, const WcsDesc &w, const WcsTab &t, int inverse, const double *in, long n, int origin, double *out, unsigned long long *counts)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_list_kernel, dim3(wcs_blocks(n)), dim3(WCS_THREADS), 0, ctx->stream, w, t, inverse, (const double2 *)in, n, origin, (double2 *)out, counts);
    return check_launch("wcs_list_kernel");
}

static int launch_wcs_pix2pix(imcom_ctx *ctx, const WcsDesc &from, const WcsTab &tf, const WcsDesc &to, const WcsTab &tt, const double *M, const double *pts, const double *grid,
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

static int launch_wcs_area_frame(imcom_ctx *ctx, const WcsDesc &w, const WcsTab &t, const double *xs, int W, const double *ys, int H, double *ra, double *dec,
                          unsigned long long *ext)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_area_frame_kernel, dim3(wcs_blocks((long)W * H)), dim3(WCS_THREADS), 0, ctx->stream, w, t, xs, W, ys, H, ra, dec, ext);
    return check_launch("wcs_area_frame_kernel");
}

static int launch_wcs_area_finish(imcom_ctx *ctx, const double *ra, const double *dec, int W, int H, int op, double pad, int rotate, double *area)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_area_finish_kernel, dim3(wcs_blocks((long)(W - 2 * op) * (H - 2 * op))), dim3(WCS_THREADS), 0, ctx->stream, ra, dec, W, H, op, pad, rotate,
                       area);
    return check_launch("wcs_area_finish_kernel");
}

static double wcs_key_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// The refusals of a packed descriptor, and the descriptor as the kernels take it.
int wcs_descriptor(const double *d, const char *who, WcsDesc *out)
{
    IMCOM_REQUIRE(d, "%s: null descriptor", who);
    for (int k = 0; k < WCS_DESC_LEN; k++) IMCOM_REQUIRE(std::isfinite(d[k]), "%s: descriptor entry %d is not finite", who, k);
    if (!(d[WCS_D_PROJ] == (double)WCS_TAN || d[WCS_D_PROJ] == (double)WCS_STG)) {
        set_error("%s: projection code %g; served are 0 (TAN, TAN-SIP) and 1 (STG)", who, d[WCS_D_PROJ]);
        return IMCOM_ERR_UNSUPPORTED;
    }
    for (int k : {WCS_D_AORDER, WCS_D_BORDER}) {
        if (!(d[k] >= 0 && d[k] == std::floor(d[k])) || d[k] > WCS_MAX_ORDER) {
            set_error("%s: a SIP order of %g; served are 0 .. %d", who, d[k], WCS_MAX_ORDER);
            return d[k] > WCS_MAX_ORDER ? IMCOM_ERR_UNSUPPORTED : IMCOM_ERR_ARG;
        }
    }
    IMCOM_REQUIRE(d[WCS_D_NITER] >= 0 && d[WCS_D_NITER] <= WCS_MAX_NITER && d[WCS_D_NITER] == std::floor(d[WCS_D_NITER]), "%s: niter = %g outside 0 .. %d", who,
                  d[WCS_D_NITER], WCS_MAX_NITER);
    IMCOM_REQUIRE(d[WCS_D_CD] * d[WCS_D_CD + 3] - d[WCS_D_CD + 1] * d[WCS_D_CD + 2] != 0.0, "%s: the CD matrix is singular", who);
    memcpy(out->d, d, sizeof(out->d));
    return IMCOM_OK;
}

// The refusals of an error table's geometry (tab == nullptr: no table, nothing to refuse).
int wcs_table_check(const void *tab, int f64, int n2, double lo, double hi, const char *who)
{
    if (!tab) return IMCOM_OK;
    IMCOM_REQUIRE(n2 >= 4 && n2 <= 32768 && lo < 0.0 && hi > (double)(n2 - 3) && std::isfinite(lo) && std::isfinite(hi) && ((uintptr_t)tab & (f64 ? 7 : 3)) == 0,
                  "%s: an error table of %d nodes an axis with end nodes %g, %g (needed: 4 .. 32768 nodes, first node < 0, last node > %d)", who, n2, lo, hi, n2 - 3);
    return IMCOM_OK;
}

// M = R_to R_from^T, row-major: native vector of `to` = M (native vector of `from`).  Every caller of wcs_pix2pix forms its M here.
void wcs_rotation_product(const WcsDesc &from, const WcsDesc &to, double *M)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += to.d[WCS_D_ROT + 3 * i + k] * from.d[WCS_D_ROT + 3 * j + k];
            M[3 * i + j] = s;
        }
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries -- the positions that set_pair's full storage holds are formed by them

namespace {

size_t wcs_table_bytes(const void *tab, int f64, int n2) { return tab ? (size_t)2 * n2 * n2 * (f64 ? 8 : 4) : 0; }

int wcs_table(Stage &st, const void *tab, int f64, int n2, double lo, double hi, const char *who, WcsTab *out)
{
    *out = WcsTab{nullptr, 0, 0, 0.0, 0.0};
    if (!tab) return IMCOM_OK;
    IMCOM_TRY(wcs_table_check(tab, f64, n2, lo, hi, who));
    const unsigned char *dev;
    IMCOM_TRY(st.in((const unsigned char *)tab, wcs_table_bytes(tab, f64, n2), &dev));
    *out = WcsTab{dev, f64 ? 1 : 0, n2, lo, hi};
    return IMCOM_OK;
}

int wcs_list(imcom_ctx *ctx, const char *who, int inverse, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *in,
             long n, int origin, double *out, long *nbad, int memspace)
{
    IMCOM_TRY(enter(ctx));
    WcsDesc w;
    IMCOM_TRY(wcs_descriptor(wcs, who, &w));
    IMCOM_REQUIRE(n >= 0 && n <= WCS_MAX_POINTS && (origin == 0 || origin == 1), "%s: %ld points (at most 2^40), origin %d", who, n, origin);
    if (nbad) *nbad = 0;
    if (n == 0) return IMCOM_OK;
    IMCOM_REQUIRE(in && out, "%s: null pointer", who);
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add(16);
    st.plan(plan, {wcs_table_bytes(tab, tab_f64, tab_n2), (size_t)n * 16, (size_t)n * 16});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *counts;
    IMCOM_TRY(ws_take(ctx, 2, &counts, who));
    WcsTab t;
    IMCOM_TRY(wcs_table(st, tab, tab_f64, tab_n2, tab_lo, tab_hi, who, &t));
    const double *in_d;
    double *out_d;
    IMCOM_TRY(st.in(in, (size_t)n * 2, &in_d));
    IMCOM_TRY(st.out(out, (size_t)n * 2, &out_d));
    if (nbad) IMCOM_HIP_CHECK(hipMemsetAsync(counts, 0, 16, ctx->stream));
    IMCOM_TRY(launch_wcs_list(ctx, w, t, inverse, in_d, n, origin, out_d, nbad ? counts : nullptr));
    IMCOM_TRY(st.back(out, out_d, (size_t)n * 2));
    if (nbad) {
        unsigned long long c[2];
        IMCOM_HIP_CHECK(hipMemcpyAsync(c, counts, 16, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *nbad = (long)c[1];
    }
    return st.done();
}
}  // namespace

extern "C" {

int imcom_wcs_sizes(long n, int W, int H, long *out)
{
    IMCOM_REQUIRE(out && n >= 0 && W >= 0 && H >= 0, "wcs_sizes: bad arguments");
    WsPlan a;
    a.add(16);
    a.add((size_t)W * H * 8);
    a.add((size_t)W * H * 8);
    out[0] = 16;               // device arrays: the two counts
    out[1] = (long)a.total;    // imcom_wcs_pix_area with device arrays: counts and the ra / dec frame
    out[2] = WCS_DESC_LEN;
    out[3] = WCS_MAX_ORDER;
    (void)n;
    return IMCOM_OK;
}

int imcom_wcs_pix2world(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *pix, long n, int origin,
                        double *world, long *nbad, int memspace)
{
    return wcs_list(ctx, "wcs_pix2world", 0, wcs, tab, tab_f64, tab_n2, tab_lo, tab_hi, pix, n, origin, world, nbad, memspace);
}

int imcom_wcs_world2pix(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *world, long n, int origin,
                        double *pix, long *nbad, int memspace)
{
    return wcs_list(ctx, "wcs_world2pix", 1, wcs, tab, tab_f64, tab_n2, tab_lo, tab_hi, world, n, origin, pix, nbad, memspace);
}

int imcom_wcs_pix2pix(imcom_ctx *ctx, const double *from, const void *ftab, int ftab_f64, int ftab_n2, double ftab_lo, double ftab_hi, const double *to, const void *ttab,
                      int ttab_f64, int ttab_n2, double ttab_lo, double ttab_hi, const double *points, const double *grid, long n, int origin, double nside, double pad,
                      void *x, void *y, int out_f32, unsigned char *is_in_ref, long *counts, int memspace)
{
    const char *who = "wcs_pix2pix";
    IMCOM_TRY(enter(ctx));
    WcsDesc wf, wt;
    IMCOM_TRY(wcs_descriptor(from, who, &wf));
    IMCOM_TRY(wcs_descriptor(to, who, &wt));
    IMCOM_REQUIRE((points != nullptr) != (grid != nullptr), "%s: either a point list or a grid", who);
    IMCOM_REQUIRE(origin == 0 || origin == 1, "%s: origin %d", who, origin);
    IMCOM_REQUIRE((x != nullptr) == (y != nullptr), "%s: x and y are given together", who);
    if (grid) {
        IMCOM_REQUIRE(grid[2] >= 0 && grid[5] >= 0 && grid[2] <= 0x7fffffff && grid[5] <= 0x7fffffff && grid[2] == std::floor(grid[2]) && grid[5] == std::floor(grid[5]),
                      "%s: a grid of %g x %g points", who, grid[5], grid[2]);
        n = (long)grid[2] * (long)grid[5];
    }
    IMCOM_REQUIRE(n >= 0 && n <= WCS_MAX_POINTS, "%s: %ld points (at most 2^40)", who, n);
    IMCOM_REQUIRE(std::isfinite(nside) && std::isfinite(pad), "%s: nside = %g, pad = %g", who, nside, pad);
    if (counts) counts[0] = counts[1] = 0;
    if (n == 0) return IMCOM_OK;
    const size_t el = out_f32 ? 4 : 8;
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add(16);
    st.plan(plan, {wcs_table_bytes(ftab, ftab_f64, ftab_n2), wcs_table_bytes(ttab, ttab_f64, ttab_n2), points ? (size_t)n * 16 : 0, x ? n * el : 0, y ? n * el : 0,
                   is_in_ref ? (size_t)n : 0});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *cnt;
    IMCOM_TRY(ws_take(ctx, 2, &cnt, who));
    WcsTab tf, tt;
    IMCOM_TRY(wcs_table(st, ftab, ftab_f64, ftab_n2, ftab_lo, ftab_hi, who, &tf));
    IMCOM_TRY(wcs_table(st, ttab, ttab_f64, ttab_n2, ttab_lo, ttab_hi, who, &tt));
    const double *pts_d;
    unsigned char *x_d, *y_d, *m_d;
    IMCOM_TRY(st.in(points, points ? (size_t)n * 2 : 0, &pts_d));
    IMCOM_TRY(st.out((unsigned char *)x, x ? n * el : 0, &x_d));
    IMCOM_TRY(st.out((unsigned char *)y, y ? n * el : 0, &y_d));
    IMCOM_TRY(st.out(is_in_ref, is_in_ref ? (size_t)n : 0, &m_d));
    double M[9];
    wcs_rotation_product(wf, wt, M);
    if (counts) IMCOM_HIP_CHECK(hipMemsetAsync(cnt, 0, 16, ctx->stream));
    IMCOM_TRY(launch_wcs_pix2pix(ctx, wf, tf, wt, tt, M, pts_d, grid, n, origin, nside, pad, x_d, y_d, out_f32, m_d, counts ? cnt : nullptr));
    if (x) IMCOM_TRY(st.back((unsigned char *)x, x_d, n * el));
    if (y) IMCOM_TRY(st.back((unsigned char *)y, y_d, n * el));
    if (is_in_ref) IMCOM_TRY(st.back(is_in_ref, m_d, (size_t)n));
    if (counts) {
        unsigned long long c[2];
        IMCOM_HIP_CHECK(hipMemcpyAsync(c, cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        counts[0] = (long)c[0], counts[1] = (long)c[1];
    }
    return st.done();
}

int imcom_wcs_pix_area(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *xs, int W, const double *ys,
                       int H, int op, double pad, double *area, int *rotated, int memspace)
{
    const char *who = "wcs_pix_area";
    IMCOM_TRY(enter(ctx));
    WcsDesc w;
    IMCOM_TRY(wcs_descriptor(wcs, who, &w));
    IMCOM_REQUIRE(xs && ys && area, "%s: null pointer", who);
    IMCOM_REQUIRE(op >= 1 && pad > 0 && W > 2 * op && H > 2 * op && (long)W * H <= 0x7fffffffL, "%s: a frame of %d x %d points with a margin of %d", who, H, W, op);
    const size_t nf = (size_t)W * H, na = (size_t)(W - 2 * op) * (H - 2 * op);
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add(16);
    plan.add(nf * 8);
    plan.add(nf * 8);
    st.plan(plan, {wcs_table_bytes(tab, tab_f64, tab_n2), (size_t)W * 8, (size_t)H * 8, na * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *ext;
    double *ra, *dec, *area_d;
    const double *xs_d, *ys_d;
    IMCOM_TRY(ws_take(ctx, 2, &ext, who));
    IMCOM_TRY(ws_take(ctx, nf, &ra, who));
    IMCOM_TRY(ws_take(ctx, nf, &dec, who));
    WcsTab t;
    IMCOM_TRY(wcs_table(st, tab, tab_f64, tab_n2, tab_lo, tab_hi, who, &t));
    IMCOM_TRY(st.in(xs, (size_t)W, &xs_d));
    IMCOM_TRY(st.in(ys, (size_t)H, &ys_d));
    IMCOM_TRY(st.out(area, na, &area_d));
    const unsigned long long init[2] = {~0ull, 0ull};
    IMCOM_TRY(upload(ctx, ext, init, 2));
    IMCOM_TRY(launch_wcs_area_frame(ctx, w, t, xs_d, W, ys_d, H, ra, dec, ext));
    unsigned long long e[2];
    IMCOM_HIP_CHECK(hipMemcpyAsync(e, ext, 16, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // wcsutil.py:740: too close to the prime meridian (a frame without a finite ra keeps its NaN)
    const int rotate = e[0] <= e[1] && wcs_key_value(e[1]) - wcs_key_value(e[0]) > 45.0;
    if (rotated) *rotated = rotate;
    IMCOM_TRY(launch_wcs_area_finish(ctx, ra, dec, W, H, op, pad, rotate, area_d));
    IMCOM_TRY(st.back(area, area_d, na));
    return st.done();
}

}  // extern "C"
