// starmom.hip -- the catalog of injected stars (reference src/pyimcom/analysis.py:1000-1057, StarsAnal.__call__, and src/pyimcom/diagnostics/
// starcube_nonoise.py:186-237): one workgroup of four waves a star.  It copies the star's cut out of the frame into LDS once (pixels outside
// the frame are zero, the np.pad of starcube_nonoise.py:194), runs the adaptive-moment iteration on it (starmom_core.h) and then, in the same
// launch, the two passes over the whole cut for the fourth moments (1016-1032) and the forced-scale moments (1035-1041).  A second, small
// kernel gives mean and np.std of the 15 x 15 windows of the maps (1044-1057), a wave a star; a third writes the cuts themselves, the cube
// of _StarCat_galsim.fits.  The C-ABI entries imcom_star_* end the file.
//
// Every sum is float64 and is reduced in one fixed order -- a thread's pixels in ascending order, the lanes of a wave by a shuffle tree, the
// four waves in order through LDS -- that depends on the cut alone, never on the grid: no atomics on floating-point values.  After a
// reduction EVERY thread reads the totals and runs the core's step in its own registers, so all 256 threads hold the same state and take
// the same exit decision; no decision is broadcast and no thread decides for the others (a workgroup whose threads disagree about leaving
// a loop with a barrier in it hangs).  The loop is bounded by max_mom2_iter + 1 and a NaN ends it through the status.
#include "launchers.h"
#include "starmom_core.h"

namespace imcom {

constexpr int SM_THREADS = 256, SM_WAVES = 4, SM_RED = 8;  // threads a star; their waves; doubles a wave in a reduction slot (>= SM_NSUMS)
constexpr int SM_HEAD = 3 * SM_WAVES * SM_RED;             // doubles of LDS in front of the cut: two slots the iterations alternate, one of the last passes

__device__ __forceinline__ double sm_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // (lane 0 holds the sum)
}

// v[0 .. N) summed over the workgroup, in every thread.  `slot`: SM_WAVES x SM_RED doubles nobody reads any more.
template <int N>
__device__ __forceinline__ void sm_block_sum(double *v, double *slot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = sm_wave_sum(v[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; i++) slot[wave * SM_RED + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = ((slot[i] + slot[SM_RED + i]) + slot[2 * SM_RED + i]) + slot[3 * SM_RED + i];
}

// frame element (r, c) or zero outside
template <typename T>
__device__ __forceinline__ T sm_frame_at(const T *__restrict__ frame, long rows, long cols, long pitch, long r, long c)
{
    return (r >= 0 && r < rows && c >= 0 && c < cols) ? frame[r * pitch + c] : (T)0;
}

template <typename T>
__global__ __launch_bounds__(SM_THREADS) void star_moments_kernel(const T *__restrict__ frame, long rows, long cols, long pitch, const int *__restrict__ ox,
                                                                  const int *__restrict__ oy, int w, int h, imcom_star_params par, double forced_scale,
                                                                  double *__restrict__ out)
{
    extern __shared__ double sm_lds[];  // SM_HEAD doubles of reduction slots, then the cut [h][w] of T
    T *cut = (T *)(sm_lds + SM_HEAD);
    const int t = threadIdx.x, k = blockIdx.x, npx = w * h;
    const long r0 = oy[k], c0 = ox[k];
    for (int i = t; i < npx; i += SM_THREADS) cut[i] = sm_frame_at(frame, rows, cols, pitch, r0 + i / w, c0 + i % w);
    __syncthreads();

    SmState s;
    sm_init(s, w, h, par);
    double sum[SM_NSUMS];
    const int tr = t >> 4, tc = t & 15;  // 16 rows at a time, 16 columns of each
    for (int it = 0; it <= par.max_mom2_iter; it++) {
        int iy1, iy2;
        if (!sm_begin(s, h, par, &iy1, &iy2)) break;  // (the same state in every thread: the same decision)
#pragma unroll
        for (int i = 0; i < SM_NSUMS; i++) sum[i] = 0.0;
        for (int iy = iy1 + tr; iy <= iy2; iy += 16) {
            double dy, b;
            int ix1, ix2;
            if (!sm_row(s, iy, w, par, &dy, &b, &ix1, &ix2)) continue;
            const T *row = cut + (iy - 1) * w;
            for (int ix = ix1 + tc; ix <= ix2; ix += 16) sm_pixel(s, ix, dy, b, (double)row[ix - 1], sum);
        }
        sm_block_sum<SM_NSUMS>(sum, sm_lds + (it & 1) * SM_WAVES * SM_RED);
        if (!sm_step(s, sum, par)) break;
    }
    if (s.status == SM_RUNNING) s.status = SM_TOO_MANY_ITERATIONS;  // (max_mom2_iter < 0)

    double col[SM_NCOL];
#pragma unroll
    for (int i = 0; i < SM_NCOL; i++) col[i] = 0.0;
    col[SMC_NITER] = (double)s.iter, col[SMC_STATUS] = (double)s.status, col[SMC_CF] = s.cf;
    if (s.status == SM_OK) {
        sm_finish(s, sum, col);
        if (forced_scale > 0.0) {
            const SmHigher hk = sm_higher(col);
            const double fs2 = forced_scale * forced_scale;
            double hs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int i = t; i < npx; i += SM_THREADS) {
                const double x_ = (double)(i % w + 1) - col[SMC_X], y_ = (double)(i / w + 1) - col[SMC_Y];
                sm_higher_pixel(hk, x_, y_, (double)cut[i], fs2, hs);
            }
            sm_block_sum<6>(hs, sm_lds + 2 * SM_WAVES * SM_RED);
            sm_higher_finish(hs, fs2, col);
        }
    }
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < SM_NCOL; i++) out[(long)k * SM_NCOL + i] = col[i];
    }
}

// a[s:e] of an axis of n elements as numpy slices it
__device__ __forceinline__ long sm_slice(long v, long n)
{
    if (v < 0) {
        v += n;
        if (v < 0) v = 0;
    }
    return v > n ? n : v;
}

__device__ __forceinline__ long long sm_wave_sum_all(long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}

// A wave a star: mean and population standard deviation of its window, in two passes.  CODED: the map holds 16-bit codes and the window is
// of table[code] (int16), summed as integers: the mean is np.mean's bit for bit.
template <typename T, bool CODED>
__global__ __launch_bounds__(SM_THREADS) void star_window_kernel(const T *__restrict__ map, long rows, long cols, long pitch, const short *__restrict__ table,
                                                                 const int *__restrict__ xi, const int *__restrict__ yi, int nstar, int bd2, double *__restrict__ out)
{
    const int k = blockIdx.x * SM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= nstar) return;  // (a whole wave)
    const long y0 = sm_slice((long)yi[k] + 1 - bd2, rows), y1 = sm_slice((long)yi[k] + bd2, rows);
    const long x0 = sm_slice((long)xi[k] + 1 - bd2, cols), x1 = sm_slice((long)xi[k] + bd2, cols);
    const long wd = x1 - x0, count = (wd > 0 && y1 > y0) ? wd * (y1 - y0) : 0;
    if (count == 0) {
        if (lane == 0) out[2 * (long)k] = out[2 * (long)k + 1] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    double mean;
    if (CODED) {
        long long isum = 0;
        for (long i = lane; i < count; i += 64) isum += table[(unsigned short)map[(y0 + i / wd) * pitch + x0 + i % wd]];
        mean = (double)sm_wave_sum_all(isum) / (double)count;
    } else {
        double fsum = 0.0;
        for (long i = lane; i < count; i += 64) fsum += (double)map[(y0 + i / wd) * pitch + x0 + i % wd];
        mean = __shfl(sm_wave_sum(fsum), 0, 64) / (double)count;
    }
    double dev = 0.0;
    for (long i = lane; i < count; i += 64) {
        const T raw = map[(y0 + i / wd) * pitch + x0 + i % wd];
        const double d = (CODED ? (double)table[(unsigned short)raw] : (double)raw) - mean;
        dev += d * d;
    }
    dev = sm_wave_sum(dev);
    if (lane == 0) out[2 * (long)k] = mean, out[2 * (long)k + 1] = sqrt(dev / (double)count);
}

template <typename T>
__global__ __launch_bounds__(SM_THREADS) void star_cuts_kernel(const T *__restrict__ frame, long rows, long cols, long pitch, const int *__restrict__ ox,
                                                               const int *__restrict__ oy, int w, int h, float *__restrict__ out)
{
    const int k = blockIdx.x, npx = w * h;
    const long r0 = oy[k], c0 = ox[k];
    for (int i = threadIdx.x; i < npx; i += SM_THREADS) out[(long)k * npx + i] = (float)sm_frame_at(frame, rows, cols, pitch, r0 + i / w, c0 + i % w);
}

// ------------------------------------------------------------------------------------------------
static size_t star_moments_lds(int w, int h, bool f64) { return (size_t)SM_HEAD * 8 + (size_t)w * h * (f64 ? 8 : 4); }

static int launch_star_moments(imcom_ctx *ctx, const void *frame, bool f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h,
                        const imcom_star_params &par, double forced_scale, double *out)
{
    ProfScope ps(ctx, "star_moments");
    const size_t lds = star_moments_lds(w, h, f64);
    if (f64) {
        if (lds > 48 * 1024) IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)star_moments_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(star_moments_kernel<double>, dim3((unsigned)nstar), dim3(SM_THREADS), lds, ctx->stream, (const double *)frame, rows, cols, pitch, ox, oy, w, h, par,
                           forced_scale, out);
    } else {
        if (lds > 48 * 1024) IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)star_moments_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(star_moments_kernel<float>, dim3((unsigned)nstar), dim3(SM_THREADS), lds, ctx->stream, (const float *)frame, rows, cols, pitch, ox, oy, w, h, par,
                           forced_scale, out);
    }
    return check_launch("star_moments_kernel");
}

static int launch_star_window_stats(imcom_ctx *ctx, const void *map, int kind, long rows, long cols, long pitch, const short *table, const int *xi, const int *yi, int nstar,
                             int bd2, double *out)
{
    ProfScope ps(ctx, "star_windows");
    const dim3 grid((unsigned)((nstar + SM_WAVES - 1) / SM_WAVES)), block(SM_THREADS);
    if (kind == 0) hipLaunchKernelGGL((star_window_kernel<float, false>), grid, block, 0, ctx->stream, (const float *)map, rows, cols, pitch, table, xi, yi, nstar, bd2, out);
    else if (kind == 1) hipLaunchKernelGGL((star_window_kernel<double, false>), grid, block, 0, ctx->stream, (const double *)map, rows, cols, pitch, table, xi, yi, nstar, bd2, out);
    else hipLaunchKernelGGL((star_window_kernel<unsigned short, true>), grid, block, 0, ctx->stream, (const unsigned short *)map, rows, cols, pitch, table, xi, yi, nstar, bd2, out);
    return check_launch("star_window_kernel");
}

static int launch_star_cuts(imcom_ctx *ctx, const void *frame, bool f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h, float *out)
{
    ProfScope ps(ctx, "star_cuts");
    if (f64) hipLaunchKernelGGL(star_cuts_kernel<double>, dim3((unsigned)nstar), dim3(SM_THREADS), 0, ctx->stream, (const double *)frame, rows, cols, pitch, ox, oy, w, h, out);
    else hipLaunchKernelGGL(star_cuts_kernel<float>, dim3((unsigned)nstar), dim3(SM_THREADS), 0, ctx->stream, (const float *)frame, rows, cols, pitch, ox, oy, w, h, out);
    return check_launch("star_cuts_kernel");
}

}  // namespace imcom

using namespace imcom;

extern "C" {

static int star_shape(const char *who, long rows, long cols, long pitch, int nstar, int w, int h)
{
    IMCOM_REQUIRE(rows >= 1 && cols >= 1 && pitch >= cols && rows <= SM_MAX_FRAME / pitch, "%s: a frame of %ld x %ld elements, pitch %ld", who, rows, cols, pitch);
    IMCOM_REQUIRE(nstar >= 0 && nstar <= (1 << 24) && w >= 1 && h >= 1, "%s: %d stars, cuts of %d x %d", who, nstar, w, h);
    if (w > SM_MAX_SIDE || h > SM_MAX_SIDE) {
        set_error("%s: cuts of %d x %d, served are sides up to %d", who, w, h, SM_MAX_SIDE);
        return IMCOM_ERR_UNSUPPORTED;
    }
    return IMCOM_OK;
}

static const imcom_star_params STAR_DEFAULTS = {1e-6, 0.25, 8000.0, 15.0, 25.0, 5.0, 400, 0};

int imcom_star_sizes(int nstar, int w, int h, int is_f64, long *out)
{
    IMCOM_REQUIRE(out, "null pointer");
    IMCOM_TRY(star_shape(__func__, 1, 1, 1, nstar, w, h));
    WsPlan plan;  // (without the frame: its size is the caller's)
    plan.add((size_t)nstar * 4);
    plan.add((size_t)nstar * 4);
    plan.add((size_t)nstar * SM_NCOL * 8);
    out[0] = (long)plan.total;
    out[1] = SM_MAX_SIDE;
    out[2] = SM_NCOL;
    out[3] = (long)star_moments_lds(w, h, is_f64 != 0);
    return IMCOM_OK;
}

int imcom_star_moments(imcom_ctx *ctx, const void *frame, int is_f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h,
                       const imcom_star_params *par, double forced_scale, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(star_shape(__func__, rows, cols, pitch, nstar, w, h));
    const imcom_star_params p = par ? *par : STAR_DEFAULTS;
    IMCOM_REQUIRE(p.max_mom2_iter >= 1 && p.max_mom2_iter <= 100000 && p.guess_sig > 0.0 && p.max_moment_nsig2 > 0.0 && p.convergence_threshold > 0.0 &&
                      p.bound_correct_wt > 0.0 && p.max_amoment > 0.0 && p.max_ashift > 0.0,
                  "star_moments: parameters out of range (every one is positive, 1 .. 100000 iterations)");
    IMCOM_REQUIRE(forced_scale == forced_scale, "star_moments: the forced scale is NaN");
    if (nstar == 0) return IMCOM_OK;
    IMCOM_REQUIRE(frame && ox && oy && out, "null pointer");
    const size_t esz = is_f64 ? 8 : 4, span = (size_t)(rows - 1) * pitch + cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * esz, (size_t)nstar * 4, (size_t)nstar * 4, (size_t)nstar * SM_NCOL * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *f_d;
    const int *x_d, *y_d;
    double *o_d;
    IMCOM_TRY(st.in((const char *)frame, span * esz, &f_d));
    IMCOM_TRY(st.in(ox, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(oy, (size_t)nstar, &y_d));
    IMCOM_TRY(st.out(out, (size_t)nstar * SM_NCOL, &o_d));
    IMCOM_TRY(launch_star_moments(ctx, f_d, is_f64 != 0, rows, cols, pitch, x_d, y_d, nstar, w, h, p, forced_scale, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)nstar * SM_NCOL));
    return st.done();
}

int imcom_star_window_stats(imcom_ctx *ctx, const void *map, int kind, long rows, long cols, long pitch, const short *table, const int *xi, const int *yi, int nstar,
                            int bd2, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(star_shape(__func__, rows, cols, pitch, nstar, 1, 1));
    IMCOM_REQUIRE(kind >= 0 && kind <= 2 && bd2 >= 1 && bd2 <= 4096, "star_window_stats: kind %d outside 0 .. 2 or bd2 = %d outside 1 .. 4096", kind, bd2);
    if (nstar == 0) return IMCOM_OK;
    IMCOM_REQUIRE(map && xi && yi && out && (kind != 2 || table), "null pointer");
    const size_t esz = kind == 1 ? 8 : kind == 0 ? 4 : 2, span = (size_t)(rows - 1) * pitch + cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * esz, kind == 2 ? (size_t)65536 * 2 : (size_t)0, (size_t)nstar * 4, (size_t)nstar * 4, (size_t)nstar * 2 * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *m_d;
    const short *t_d = nullptr;
    const int *x_d, *y_d;
    double *o_d;
    IMCOM_TRY(st.in((const char *)map, span * esz, &m_d));
    if (kind == 2) IMCOM_TRY(st.in(table, (size_t)65536, &t_d));
    IMCOM_TRY(st.in(xi, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(yi, (size_t)nstar, &y_d));
    IMCOM_TRY(st.out(out, (size_t)nstar * 2, &o_d));
    IMCOM_TRY(launch_star_window_stats(ctx, m_d, kind, rows, cols, pitch, t_d, x_d, y_d, nstar, bd2, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)nstar * 2));
    return st.done();
}

int imcom_star_cuts(imcom_ctx *ctx, const void *frame, int is_f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h, float *out,
                    int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(star_shape(__func__, rows, cols, pitch, nstar, w, h));
    if (nstar == 0) return IMCOM_OK;
    IMCOM_REQUIRE(frame && ox && oy && out, "null pointer");
    const size_t esz = is_f64 ? 8 : 4, span = (size_t)(rows - 1) * pitch + cols, nout = (size_t)nstar * w * h;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * esz, (size_t)nstar * 4, (size_t)nstar * 4, nout * 4});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *f_d;
    const int *x_d, *y_d;
    float *o_d;
    IMCOM_TRY(st.in((const char *)frame, span * esz, &f_d));
    IMCOM_TRY(st.in(ox, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(oy, (size_t)nstar, &y_d));
    IMCOM_TRY(st.out(out, nout, &o_d));
    IMCOM_TRY(launch_star_cuts(ctx, f_d, is_f64 != 0, rows, cols, pitch, x_d, y_d, nstar, w, h, o_d));
    IMCOM_TRY(st.back(out, (const float *)o_d, nout));
    return st.done();
}

}  // extern "C"
