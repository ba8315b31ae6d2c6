// wcs.hip -- world coordinate systems on the device: the closed arithmetic that the reference's PyIMCOM_WCS reduces a WCS to
// (src/pyimcom/wcsutil.py:419-634: a FITS TAN-SIP header, or for gwcs input a fitted TAN-SIP plus a bilinear error map), the pixel ->
// pixel map of compareutils.map_sca2sca (src/pyimcom/utils/compareutils.py:63-106) and the pixel areas of wcsutil.get_pix_area
// (wcsutil.py:688-788).  The per-point arithmetic is wcs_core.h's.
//
// One thread owns a point (WCS_ITEMS points, a workgroup's tile apart, so that a wave's store is contiguous).  The descriptors travel as
// kernel arguments, so every coefficient is wave-uniform; the only gathers are the eight taps of an error-table look-up (four in each of its two
// planes).
// Counts are summed as integers inside a workgroup and added once a workgroup; there is no float atomic and no float sum across threads, so
// the results are the same bits for every run and every chunking.  The C entries imcom_wcs_* follow the kernels; the HEALPix star grids
// (seam 18), which end in wcs_world2pix, and their entries imcom_healpix_* end the file.
#include <algorithm>

#include "launchers.h"
#include "wcs_core.h"
#include "healpix_core.h"

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

// Sca_img's effective gain (imdestripe.py:281-297) from the frame of wcs_area_frame_kernel, ra and dec [n + 2][n + 2] in degrees of the pixels
// -1 .. n (get_coordinates(pad=2.0), 451-474): the centred differences, their determinant, 1 / (|det| cos(dec)).  No turn away from the prime
// meridian: the reference has none here.  The reference transposes its stack of derivatives before it takes the determinants (292-293), so
// gain[i][j] has the determinant of pixel (row j, column i) and the cosine of pixel (row i, column j); that is kept.
__global__ __launch_bounds__(WCS_THREADS) void wcs_gain_finish_kernel(const double *__restrict__ ra, const double *__restrict__ dec, int n, void *__restrict__ gain, int f32)
{
    const long W = n + 2, total = (long)n * n, p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < WCS_ITEMS; k++) {
        const long p = p0 + (long)k * WCS_THREADS;
        if (p >= total) break;
        const long i = p / n, j = p - i * n;
        const long c = (j + 1) * W + (i + 1);  // frame index of pixel (row j, column i)
        const double rx = (ra[c + 1] - ra[c - 1]) / 2.0, ry = (ra[c + W] - ra[c - W]) / 2.0;
        const double dx = (dec[c + 1] - dec[c - 1]) / 2.0, dy = (dec[c + W] - dec[c - W]) / 2.0;
        const double det = rx * dy - ry * dx;
        const double g = 1.0 / (fabs(det) * cos(dec[(i + 1) * W + (j + 1)] * WCS_DEG));
        if (f32) ((float *)gain)[p] = (float)g;
        else ((double *)gain)[p] = g;
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

static int launch_wcs_gain_finish(imcom_ctx *ctx, const double *ra, const double *dec, int n, void *gain, int f32)
{
    ProfScope ps(ctx, "wcs");
    hipLaunchKernelGGL(wcs_gain_finish_kernel, dim3(wcs_blocks((long)n * n)), dim3(WCS_THREADS), 0, ctx->stream, ra, dec, n, gain, f32);
    return check_launch("wcs_gain_finish_kernel");
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

// The workspace of imcom_wcs_effective_gain with device arrays: the extremes, the ra and dec frames of (nside + 2)^2 points, the axis.
size_t wcs_gain_ws_bytes(int nside)
{
    const size_t W = (size_t)nside + 2;
    WsPlan plan;
    plan.add(16);
    plan.add(W * W * 8);
    plan.add(W * W * 8);
    plan.add(W * 8);
    return plan.total;
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

// ---------------------------------------------------------------------------------------------
// HEALPix star grids (seam 18): the pixels of the RING scheme inside a circle on the sky, their centres, and those centres through a WCS --
// GridInject.make_sph_grid / generate_star_grid (src/pyimcom/layer.py:690-789), and healpy's query_disc + pix2ang + all_world2pix of
// StarsAnal.__call__ (analysis.py:957-978), gen_starcube_nonoise (starcube_nonoise.py:145-175), gen_dynrange_data (dynrange.py:167-191) and
// gen_truthcats (truthcats.py:190-241).  The per-pixel arithmetic is healpix_core.h's.
//
// The cap: one workgroup owns one ring of the range and strides that ring's phi window.  A first pass counts the ring's hits (a ballot and a
// population count a wave, one LDS slot a wave), one workgroup scans the ring counts, and a second pass with the same traversal writes every
// hit at (ring offset + rank in ring).  The output ascends in the pixel index; there is no atomic, so the bits do not depend on the run.

namespace imcom {

namespace {

constexpr int HP_THREADS = 256;
constexpr long HP_MAX_RINGS = 1L << 22;  // most rings of one cap (a workgroup a ring; the scan is one workgroup's)

struct HpCapArgs {
    int res, lonlat, origin, has_wcs, box_n, box_bdpad;
    long ring0, plo, phi, capacity;  // the first ring; the pixel range, both ends included; the room of the outputs
    double ra, ra_window, sd, cd, cosr, radius, theta0, s0;
};

struct HpCapOut {
    long *ipix;
    double *ra, *dec, *ra_deg, *dec_deg, *x, *y, *pa;
};

struct HpHit {
    long p;
    double phi, lon, lat, x, y;
};

// Whether index j of ring g belongs to the selection; h: the pixel, its centre in degrees and (with a WCS, when the box or the output needs
// it) its position.
template <bool FILL>
__device__ __forceinline__ bool hp_cap_test(const HpCapArgs &a, const WcsDesc &w, const WcsTab &t, const HpRing &g, double theta, long j, HpHit *h)
{
    const long p = g.start + j;
    if (p < a.plo || p > a.phi) return false;
    const double phi = hp_ring_phi(g, j);
    if (!(hp_cap_mu(a.sd, a.cd, a.ra, theta, phi) >= a.cosr)) return false;
    h->p = p, h->phi = phi;
    if (!FILL && a.box_n <= 0) return true;
    hp_degrees(theta, phi, a.lonlat, &h->lon, &h->lat);
    if (!a.has_wcs) return true;
    wcs_world2pix(w, t, h->lon, h->lat, a.origin, &h->x, &h->y);
    return a.box_n <= 0 || (hp_in_box(h->x, a.box_n, a.box_bdpad) && hp_in_box(h->y, a.box_n, a.box_bdpad));
}

// FILL false: counts[ring] = the ring's hits.  FILL true: the hits at offsets[ring] + rank in ring.
template <bool FILL>
__global__ __launch_bounds__(HP_THREADS) void hp_cap_kernel(const HpCapArgs a, const WcsDesc w, const WcsTab t, unsigned *__restrict__ counts,
                                                           const long *__restrict__ offsets, const HpCapOut o)
{
    __shared__ unsigned wcnt[HP_THREADS / 64];
    HpRing g;
    hp_ring_info(a.res, a.ring0 + (long)blockIdx.x, &g);
    double z, sth;
    const double theta = hp_ring_theta(a.res, g.ring, &z, &sth);
    int64_t first, count;
    hp_ring_window(theta, sth, a.theta0, a.s0, a.radius, a.ra_window, g, &first, &count);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = FILL ? offsets[blockIdx.x] : 0;
    unsigned total = 0;
#pragma unroll 1
    for (long k0 = 0; k0 < count; k0 += HP_THREADS) {  // (count is the workgroup's: every thread makes every trip)
        const long k = k0 + threadIdx.x;
        HpHit h;
        const bool hit = k < count && hp_cap_test<FILL>(a, w, t, g, theta, hp_window_index(g, first, count, k), &h);
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int q = 0; q < HP_THREADS / 64; q++) {
            before += q < wave ? wcnt[q] : 0u;
            all += wcnt[q];
        }
        if (FILL && hit) {
            const long at = base + total + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (at < a.capacity) {
                if (o.ipix) o.ipix[at] = h.p;
                if (o.ra) o.ra[at] = h.phi;
                if (o.dec) o.dec[at] = HP_HALFPI - theta;
                if (o.ra_deg) o.ra_deg[at] = h.lon;
                if (o.dec_deg) o.dec_deg[at] = h.lat;
                if (o.x) o.x[at] = h.x, o.y[at] = h.y;
                if (o.pa) {  // truthcats.py:229-241: the direction of north at +- 1 arcsec
                    double xpp, ypp, xmm, ymm;
                    wcs_world2pix(w, t, h.lon, h.lat + 1.0 / 3600.0, a.origin, &xpp, &ypp);
                    wcs_world2pix(w, t, h.lon, h.lat - 1.0 / 3600.0, a.origin, &xmm, &ymm);
                    o.pa[at] = hp_position_angle(xpp, ypp, xmm, ymm);
                }
            }
        }
        total += all;
        __syncthreads();
    }
    if (!FILL && threadIdx.x == 0) counts[blockIdx.x] = total;
}

// offsets [n + 1] = the exclusive prefix sums of counts [n] and their total: one workgroup, every thread a contiguous share.
__global__ __launch_bounds__(HP_THREADS) void hp_ring_scan_kernel(const unsigned *__restrict__ counts, long n, long *__restrict__ offsets)
{
    __shared__ long part[HP_THREADS];
    const long share = (n + HP_THREADS - 1) / HP_THREADS, lo = (long)threadIdx.x * share, hi = lo + share < n ? lo + share : n;
    long s = 0;
    for (long k = lo; k < hi; k++) s += counts[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long run = 0;
        for (int q = 0; q < HP_THREADS; q++) {
            const long c = part[q];
            part[q] = run;
            run += c;
        }
        offsets[n] = run;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (long k = lo; k < hi; k++) {
        offsets[k] = s;
        s += counts[k];
    }
}

// ipix [n] -> (theta, phi) in radians or (lonlat) (lon, lat) in degrees; a pixel outside 0 .. npix - 1 gives NaN and is counted in bad[1].
__global__ __launch_bounds__(WCS_THREADS) void hp_pix2ang_kernel(int res, const long *__restrict__ ipix, long n, int lonlat, double *__restrict__ a, double *__restrict__ b,
                                                                unsigned long long *bad)
{
    unsigned nbad = 0;
    const long p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x, npix = hp_npix(res);
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long k = p0 + (long)i * WCS_THREADS;
        if (k >= n) break;
        const long p = ipix[k];
        double theta = NAN, phi = NAN;
        if (p >= 0 && p < npix) {
            hp_pix2ang(res, p, &theta, &phi);
            if (lonlat) hp_degrees(theta, phi, 1, &phi, &theta);  // (lon, lat) take the places of (phi, theta)
        } else {
            nbad++;
        }
        a[k] = lonlat ? phi : theta;
        b[k] = lonlat ? theta : phi;
    }
    wcs_block_counts(0u, nbad, bad);
}

// (theta, phi) in radians, or (lonlat) (lon, lat) in degrees as healpy turns them (theta = pi / 2 - radians(lat), phi = radians(lon)), ->
// ipix [n]; an angle that is not finite or a colatitude outside [0, pi] gives -1 and is counted in bad[1].
__global__ __launch_bounds__(WCS_THREADS) void hp_ang2pix_kernel(int res, const double *__restrict__ a, const double *__restrict__ b, long n, int lonlat,
                                                                long *__restrict__ ipix, unsigned long long *bad)
{
    unsigned nbad = 0;
    const long p0 = (long)blockIdx.x * WCS_TILE + threadIdx.x;
#pragma unroll 1
    for (int i = 0; i < WCS_ITEMS; i++) {
        const long k = p0 + (long)i * WCS_THREADS;
        if (k >= n) break;
        double theta = a[k], phi = b[k];
        if (lonlat) {
            HP_SEPARATE_ROUNDINGS
            const double lat = b[k] * HP_DEG;
            phi = a[k] * HP_DEG, theta = HP_HALFPI - lat;
        }
        long p = -1;
        if (theta - theta == 0.0 && phi - phi == 0.0 && theta >= 0.0 && theta <= HP_PI) p = hp_ang2pix(res, theta, phi);
        else nbad++;
        ipix[k] = p;
    }
    wcs_block_counts(0u, nbad, bad);
}

}  // namespace

}  // namespace imcom

namespace {

int healpix_list(imcom_ctx *ctx, const char *who, int inverse, int res, const void *in_a, const void *in_b, long n, int lonlat, void *out_a, void *out_b, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(res >= 0 && res <= HP_MAX_RES && n >= 0 && n <= WCS_MAX_POINTS && (lonlat == 0 || lonlat == 1), "%s: res %d (0 .. %d), %ld points, lonlat %d", who, res,
                  HP_MAX_RES, n, lonlat);
    if (n == 0) return IMCOM_OK;
    IMCOM_REQUIRE(in_a && out_a && (inverse ? in_b != nullptr : out_b != nullptr), "%s: null pointer", who);
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add(16);
    st.plan(plan, {(size_t)n * 8, inverse ? (size_t)n * 8 : 0, (size_t)n * 8, inverse ? 0 : (size_t)n * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *counts;
    IMCOM_TRY(ws_take(ctx, 2, &counts, who));
    const double *ia, *ib;
    double *oa, *ob;
    IMCOM_TRY(st.in((const double *)in_a, (size_t)n, &ia));  // (eight bytes an element either way)
    IMCOM_TRY(st.in((const double *)in_b, inverse ? (size_t)n : 0, &ib));
    IMCOM_TRY(st.out((double *)out_a, (size_t)n, &oa));
    IMCOM_TRY(st.out((double *)out_b, inverse ? 0 : (size_t)n, &ob));
    IMCOM_HIP_CHECK(hipMemsetAsync(counts, 0, 16, ctx->stream));
    {
        ProfScope ps(ctx, "healpix");
        if (inverse) hipLaunchKernelGGL(hp_ang2pix_kernel, dim3(wcs_blocks(n)), dim3(WCS_THREADS), 0, ctx->stream, res, ia, ib, n, lonlat, (long *)oa, counts);
        else hipLaunchKernelGGL(hp_pix2ang_kernel, dim3(wcs_blocks(n)), dim3(WCS_THREADS), 0, ctx->stream, res, (const long *)ia, n, lonlat, oa, ob, counts);
        IMCOM_TRY(check_launch(inverse ? "hp_ang2pix_kernel" : "hp_pix2ang_kernel"));
    }
    IMCOM_TRY(st.back((double *)out_a, oa, (size_t)n));
    IMCOM_TRY(st.back((double *)out_b, ob, inverse ? 0 : (size_t)n));
    unsigned long long c[2];
    IMCOM_HIP_CHECK(hipMemcpyAsync(c, counts, 16, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMCOM_REQUIRE(c[1] == 0, inverse ? "%s: %llu angles that are not finite or whose colatitude is outside [0, pi]" : "%s: %llu pixels outside 0 .. 12 * 4^res - 1", who, c[1]);
    return IMCOM_OK;
}

}  // namespace

extern "C" {

int imcom_healpix_pix2ang(imcom_ctx *ctx, int res, const long *ipix, long n, int lonlat, double *a, double *b, int memspace)
{
    return healpix_list(ctx, "healpix_pix2ang", 0, res, ipix, nullptr, n, lonlat, a, b, memspace);
}

int imcom_healpix_ang2pix(imcom_ctx *ctx, int res, const double *a, const double *b, long n, int lonlat, long *ipix, int memspace)
{
    return healpix_list(ctx, "healpix_ang2pix", 1, res, a, b, n, lonlat, ipix, nullptr, memspace);
}

int imcom_healpix_cap(imcom_ctx *ctx, int res, double ra, double dec, double radius, int mode, int lonlat, const double *wcs, const void *tab, int tab_f64, int tab_n2,
                      double tab_lo, double tab_hi, int origin, int box_n, int box_bdpad, long capacity, long *ipix, double *ra_pix, double *dec_pix, double *ra_deg,
                      double *dec_deg, double *x, double *y, double *pa, long *count, int memspace)
{
    const char *who = "healpix_cap";
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(res >= 0 && res <= HP_MAX_RES && (mode == 0 || mode == 1) && (lonlat == 0 || lonlat == 1), "%s: res %d (0 .. %d), mode %d, lonlat %d", who, res,
                  HP_MAX_RES, mode, lonlat);
    IMCOM_REQUIRE(std::isfinite(ra) && std::fabs(dec) <= HP_HALFPI && radius >= 0.0 && radius <= HP_PI, "%s: centre (%g, %g) rad, radius %g rad", who, ra, dec, radius);
    IMCOM_REQUIRE((x != nullptr) == (y != nullptr), "%s: x and y are given together", who);
    IMCOM_REQUIRE(wcs || (!x && !pa && box_n <= 0), "%s: positions, the box and the position angle need a WCS", who);
    IMCOM_REQUIRE(origin == 0 || origin == 1, "%s: origin %d", who, origin);
    IMCOM_REQUIRE(box_n <= 0 || (box_bdpad >= 0 && 2L * box_bdpad < box_n), "%s: a box of %d pixels with a border of %d", who, box_n, box_bdpad);
    const bool fill = ipix || ra_pix || dec_pix || ra_deg || dec_deg || x || pa;
    IMCOM_REQUIRE(fill || count, "%s: nothing to return", who);
    IMCOM_REQUIRE(!fill || capacity >= 0, "%s: room for %ld pixels", who, capacity);
    HpCapArgs a = {};
    WcsDesc w = {};
    if (wcs) IMCOM_TRY(wcs_descriptor(wcs, who, &w));
    a.res = res, a.lonlat = lonlat, a.origin = origin, a.has_wcs = wcs ? 1 : 0, a.box_n = box_n > 0 ? box_n : 0, a.box_bdpad = box_bdpad;
    a.ra = ra, a.ra_window = hp_fmodulo(ra, HP_TWOPI), a.sd = std::sin(dec), a.cd = std::cos(dec), a.cosr = std::cos(radius), a.radius = radius;
    a.theta0 = HP_HALFPI - dec, a.s0 = a.cd > 0.0 ? a.cd : 0.0, a.capacity = fill ? capacity : 0;
    int64_t pmin, pmax;
    hp_cap_range(res, ra, dec, radius, &pmin, &pmax);
    HpRing g0, g1;
    hp_ring_info(res, hp_pix2ring(res, pmin), &g0);
    hp_ring_info(res, hp_pix2ring(res, pmax), &g1);
    const long nrings = (long)(g1.ring - g0.ring + 1);
    IMCOM_REQUIRE(nrings >= 1 && nrings <= HP_MAX_RINGS, "%s: the cap spans %ld rings (at most %ld)", who, nrings, HP_MAX_RINGS);
    a.ring0 = g0.ring;
    a.plo = mode ? g0.start : pmin, a.phi = mode ? g1.start + g1.len - 1 : pmax;  // the full disc takes whole rings
    const size_t cap = fill ? (size_t)capacity : 0;
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add((size_t)nrings * 4);
    plan.add((size_t)(nrings + 1) * 8);
    st.plan(plan, {wcs_table_bytes(wcs ? tab : nullptr, tab_f64, tab_n2), ipix ? cap * 8 : 0, ra_pix ? cap * 8 : 0, dec_pix ? cap * 8 : 0, ra_deg ? cap * 8 : 0,
                   dec_deg ? cap * 8 : 0, x ? cap * 8 : 0, y ? cap * 8 : 0, pa ? cap * 8 : 0});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned *counts;
    long *offsets;
    IMCOM_TRY(ws_take(ctx, (size_t)nrings, &counts, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nrings + 1, &offsets, who));
    WcsTab t;
    IMCOM_TRY(wcs_table(st, wcs ? tab : nullptr, tab_f64, tab_n2, tab_lo, tab_hi, who, &t));
    HpCapOut o = {};
    IMCOM_TRY(st.out(ipix, ipix ? cap : 0, &o.ipix));
    IMCOM_TRY(st.out(ra_pix, ra_pix ? cap : 0, &o.ra));
    IMCOM_TRY(st.out(dec_pix, dec_pix ? cap : 0, &o.dec));
    IMCOM_TRY(st.out(ra_deg, ra_deg ? cap : 0, &o.ra_deg));
    IMCOM_TRY(st.out(dec_deg, dec_deg ? cap : 0, &o.dec_deg));
    IMCOM_TRY(st.out(x, x ? cap : 0, &o.x));
    IMCOM_TRY(st.out(y, y ? cap : 0, &o.y));
    IMCOM_TRY(st.out(pa, pa ? cap : 0, &o.pa));
    long total = 0;
    {
        ProfScope ps(ctx, "healpix", 2);
        hipLaunchKernelGGL(hp_cap_kernel<false>, dim3((unsigned)nrings), dim3(HP_THREADS), 0, ctx->stream, a, w, t, counts, (const long *)nullptr, HpCapOut{});
        IMCOM_TRY(check_launch("hp_cap_kernel (count)"));
        hipLaunchKernelGGL(hp_ring_scan_kernel, dim3(1), dim3(HP_THREADS), 0, ctx->stream, (const unsigned *)counts, nrings, offsets);
        IMCOM_TRY(check_launch("hp_ring_scan_kernel"));
    }
    IMCOM_HIP_CHECK(hipMemcpyAsync(&total, offsets + nrings, 8, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (count) *count = total;
    if (!fill) return IMCOM_OK;
    IMCOM_REQUIRE(total == capacity, "%s: the selection holds %ld pixels and the outputs have room for %ld", who, total, capacity);
    if (total == 0) return IMCOM_OK;
    {
        ProfScope ps(ctx, "healpix");
        hipLaunchKernelGGL(hp_cap_kernel<true>, dim3((unsigned)nrings), dim3(HP_THREADS), 0, ctx->stream, a, w, t, (unsigned *)nullptr, (const long *)offsets, o);
        IMCOM_TRY(check_launch("hp_cap_kernel (fill)"));
    }
    IMCOM_TRY(st.back(ipix, o.ipix, ipix ? cap : 0));
    IMCOM_TRY(st.back(ra_pix, o.ra, ra_pix ? cap : 0));
    IMCOM_TRY(st.back(dec_pix, o.dec, dec_pix ? cap : 0));
    IMCOM_TRY(st.back(ra_deg, o.ra_deg, ra_deg ? cap : 0));
    IMCOM_TRY(st.back(dec_deg, o.dec_deg, dec_deg ? cap : 0));
    IMCOM_TRY(st.back(x, o.x, x ? cap : 0));
    IMCOM_TRY(st.back(y, o.y, y ? cap : 0));
    IMCOM_TRY(st.back(pa, o.pa, pa ? cap : 0));
    return st.done();
}

// Seam 21: the effective gain of an SCA of nside x nside pixels from its WCS (imdestripe.py:281-297), float32 (out_f32) or float64
// [nside][nside].
int imcom_wcs_effective_gain(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, int nside, void *gain,
                             int out_f32, int memspace)
{
    const char *who = "wcs_effective_gain";
    IMCOM_TRY(enter(ctx));
    WcsDesc w;
    IMCOM_TRY(wcs_descriptor(wcs, who, &w));
    IMCOM_REQUIRE(nside >= 1 && nside <= 32768 && gain, "%s: an SCA of %d pixels a side, or a null output", who, nside);
    const int W = nside + 2;
    const size_t nf = (size_t)W * W, ng = (size_t)nside * nside, el = out_f32 ? 4 : 8;
    WsPlan plan;
    plan.add(wcs_gain_ws_bytes(nside));
    Stage st(ctx, memspace, who);
    st.plan(plan, {wcs_table_bytes(tab, tab_f64, tab_n2), ng * el});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *ext;
    double *ra, *dec, *axis;
    IMCOM_TRY(ws_take(ctx, 2, &ext, who));
    IMCOM_TRY(ws_take(ctx, nf, &ra, who));
    IMCOM_TRY(ws_take(ctx, nf, &dec, who));
    IMCOM_TRY(ws_take(ctx, (size_t)W, &axis, who));
    WcsTab t;
    IMCOM_TRY(wcs_table(st, tab, tab_f64, tab_n2, tab_lo, tab_hi, who, &t));
    unsigned char *gain_d;
    IMCOM_TRY(st.out((unsigned char *)gain, ng * el, &gain_d));
    std::vector<double> pix((size_t)W);
    for (int k = 0; k < W; k++) pix[k] = (double)k - 1.0;  // 468-470: arange(nside + 2) - 2 / 2
    IMCOM_TRY(upload(ctx, axis, pix.data(), pix.size()));
    const unsigned long long init[2] = {~0ull, 0ull};
    IMCOM_TRY(upload(ctx, ext, init, 2));
    IMCOM_TRY(launch_wcs_area_frame(ctx, w, t, axis, W, axis, W, ra, dec, ext));
    IMCOM_TRY(launch_wcs_gain_finish(ctx, ra, dec, nside, gain_d, out_f32 ? 1 : 0));
    IMCOM_TRY(st.back((unsigned char *)gain, gain_d, ng * el));
    return st.done();
}

}  // extern "C"
