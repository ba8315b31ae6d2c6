// objmask.hip -- the bright-object mask of the destripe set-up (reference src/pyimcom/imdestripe.py:781-872, apply_object_mask, and its
// caller Sca_img.__init__ 317-332): exact order statistics of a device array, threshold and clipping flags, constrained propagation of a
// binary image (scipy.ndimage.binary_propagation, 4-connectivity, border 0), box dilation (binary_dilation with (2r+1)^2 ones) and the
// application of the mask.  The C-ABI entries imcom_select_kth / imcom_mask_* end the file.
//
// Every result is a boolean image, an integer count or an order statistic: integer arithmetic and comparisons only, so each has one right
// value, whatever the cut into threads and workgroups and from run to run.  Masks are uint8 images, one byte a pixel, as everywhere in the
// library; inside a workgroup they are bit rows in LDS, one 64-bit word a row.
#include <algorithm>

#include "launchers.h"
#include "objmask_core.h"

namespace imcom {

constexpr int SELECT_BINS = 2048, SELECT_STATE = 8;  // histogram bins of a pass (two histograms); words of the selection state
constexpr int MASK_DILATE_TX = 48, MASK_DILATE_TY = 32, MASK_DILATE_MAX_R = 8;  // output pixels of a dilation workgroup; largest radius
constexpr int MASK_PROPAGATE_T = 62;                                            // side of a propagation tile

__device__ __forceinline__ float om_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double om_abs(double v) { return fabs(v); }

// ------------------------------------------------------------------------------------------------
// Selection.  The k-th smallest of the flagged values (or of |v - c|, formed here and never stored) by radix select on their keys: a pass
// counts, per digit value, the elements whose higher digits equal the prefix decided so far; select_pick_kernel walks the counts to the
// digit that holds the rank and lengthens the prefix.  Two ranks ride together (the two middle ones of an even count): while their
// prefixes agree one histogram serves both.  state [SELECT_STATE] (device): prefix 0 / 1, rank 0 / 1 within the prefix, the number of
// values that are not NaN, the number that are, and a word per rank that says "the answer is NaN" (the rank lies among the NaNs, which
// sort last as in numpy, or nothing is flagged).  hist [2][OM_BINS].  All counts are integers added with atomics: the same in any order.
template <typename T>
__global__ __launch_bounds__(256) void select_hist_kernel(const T *__restrict__ vals, const unsigned char *__restrict__ flags, long n, int use_abs, T c, int pass,
                                                          unsigned long long *__restrict__ state, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int h[2][OM_BINS];
    __shared__ unsigned int nan_lds;
    const int t = threadIdx.x;
    for (int b = t; b < 2 * OM_BINS; b += 256) (&h[0][0])[b] = 0;
    if (t == 0) nan_lds = 0;
    __syncthreads();
    int shift, nbits;
    om_digit(8 * (int)sizeof(T), pass, &shift, &nbits);
    const int top = shift + nbits;
    const unsigned long long p0 = state[0], p1 = state[1];
    const bool live0 = state[6] == 0, live1 = state[7] == 0 && p1 != p0;  // (equal prefixes: the first histogram is both)
    const unsigned long long hi0 = top >= 64 ? 0ull : p0 >> top, hi1 = top >= 64 ? 0ull : p1 >> top;
    const unsigned dmask = (1u << nbits) - 1u;
    // a thread adds a run of equal digits at once: an image of sky has long ones
    int last0 = -1, last1 = -1;
    unsigned run0 = 0, run1 = 0, nans = 0;
    for (long i = (long)blockIdx.x * 256 + t; i < n; i += (long)gridDim.x * 256) {
        if (flags && !flags[i]) continue;
        T v = vals[i];
        if (use_abs) v = om_abs(v - c);
        if (v != v) {
            nans++;
            continue;
        }
        const unsigned long long key = om_key(v), hi = top >= 64 ? 0ull : key >> top;
        const int d = (int)((unsigned)(key >> shift) & dmask);
        if (live0 && hi == hi0) {
            if (d == last0) run0++;
            else {
                if (run0) atomicAdd(&h[0][last0], run0);
                last0 = d, run0 = 1;
            }
        }
        if (live1 && hi == hi1) {
            if (d == last1) run1++;
            else {
                if (run1) atomicAdd(&h[1][last1], run1);
                last1 = d, run1 = 1;
            }
        }
    }
    if (run0) atomicAdd(&h[0][last0], run0);
    if (run1) atomicAdd(&h[1][last1], run1);
    if (pass == 0 && nans) atomicAdd(&nan_lds, nans);
    __syncthreads();
    for (int b = t; b < 2 * OM_BINS; b += 256) {
        const unsigned v = (&h[0][0])[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
    if (t == 0 && nan_lds) atomicAdd(&state[5], (unsigned long long)nan_lds);
}

// One workgroup: takes the histograms (and zeroes them for the next pass), fixes the ranks after pass 0 (k < 0: the two middle ones of the
// m flagged values, else k and min(k + 1, m - 1)), finds each rank's digit.  The last pass writes res: the two values in the array's type
// (NaN where the rank lies among the NaNs) and info = {m, number of NaNs}.
__global__ __launch_bounds__(256) void select_pick_kernel(int is_f64, int pass, long k, unsigned long long *__restrict__ state, unsigned long long *__restrict__ hist,
                                                          void *__restrict__ res, long *__restrict__ info)
{
    __shared__ unsigned long long h[2][OM_BINS];
    const int t = threadIdx.x, keybits = is_f64 ? 64 : 32;
    const bool same = state[0] == state[1];
    for (int b = t; b < OM_BINS; b += 256) {
        h[0][b] = hist[b];
        h[1][b] = same ? hist[b] : hist[OM_BINS + b];
        hist[b] = 0;
        hist[OM_BINS + b] = 0;
    }
    __syncthreads();
    if (t != 0) return;
    int shift, nbits;
    om_digit(keybits, pass, &shift, &nbits);
    if (pass == 0) {
        unsigned long long real = 0;
        for (int b = 0; b < OM_BINS; b++) real += h[0][b];
        const unsigned long long m = real + state[5];
        state[4] = real;
        unsigned long long r0 = 0, r1 = 0;
        if (m > 0) {
            r0 = k < 0 ? (m - 1) / 2 : (unsigned long long)k;
            r1 = k < 0 ? m / 2 : ((unsigned long long)k + 1 < m ? (unsigned long long)k + 1 : m - 1);
        }
        state[2] = r0, state[3] = r1;
        state[6] = (m == 0 || r0 >= real) ? 1 : 0;
        state[7] = (m == 0 || r1 >= real) ? 1 : 0;
    }
    for (int r = 0; r < 2; r++) {
        if (state[6 + r]) continue;
        const unsigned long long rank = state[2 + r];
        unsigned long long cum = 0;
        int d = 0;
        const int bins = 1 << nbits;
        while (d < bins - 1 && cum + h[r][d] <= rank) cum += h[r][d++];
        state[2 + r] = rank - cum;
        state[r] |= (unsigned long long)d << shift;
    }
    if (pass == om_passes(keybits) - 1) {
        for (int r = 0; r < 2; r++) {
            if (is_f64) ((double *)res)[r] = state[6 + r] ? __longlong_as_double(0x7FF8000000000000ll) : om_value_f64(state[r]);
            else ((float *)res)[r] = state[6 + r] ? __uint_as_float(0x7FC00000u) : om_value_f32(state[r]);
        }
        info[0] = (long)(state[4] + state[5]);
        info[1] = (long)state[5];
    }
}

// ------------------------------------------------------------------------------------------------
// Flags.  Differences are formed in the image's type (numpy's `image - bkg`), compared as doubles: exact for both types, and it serves
// the float32 image compared with a float64 scalar, which numpy compares in float64.
template <typename T>
__global__ __launch_bounds__(256) void mask_threshold_kernel(const T *__restrict__ img, long n, T bkg, double t1, double t2, int finite_only,
                                                             unsigned char *__restrict__ m1, unsigned char *__restrict__ m2)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T v = img[i];
    const bool ok = !finite_only || isfinite(v);
    const double d = (double)(T)(v - bkg);
    m1[i] = (ok && d >= t1) ? 1 : 0;  // (a NaN compares false)
    if (m2) m2[i] = (ok && d >= t2) ? 1 : 0;
}

// keep_out = keep_in && |v - bkg| < t, or isfinite(v) without a keep_in; *count += the number kept
template <typename T>
__global__ __launch_bounds__(256) void mask_clip_kernel(const T *__restrict__ img, long n, const unsigned char *keep_in, T bkg, double t,
                                                        unsigned char *keep_out, unsigned long long *__restrict__ count)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) {
        const T v = img[i];
        k = keep_in ? (keep_in[i] != 0 && (double)om_abs((T)(v - bkg)) < t) : (bool)isfinite(v);
        keep_out[i] = k ? 1 : 0;
    }
    const int c = __syncthreads_count(k ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(count, (unsigned long long)c);
}

template <typename T>
__global__ __launch_bounds__(256) void mask_apply_kernel(const T *in, const unsigned char *mask, long n, T *out)  // (out may be in)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = mask[i] ? (T)0 : in[i];
}

// ------------------------------------------------------------------------------------------------
// Box dilation of radius r <= MASK_DILATE_MAX_R, border 0.  A workgroup owns MASK_DILATE_TX x MASK_DILATE_TY output pixels and reads the
// 64 x 48 window around them (halo 8) as bit rows: thread q forms one byte of a row word, as in pcg64.hip.  A row is smeared r bits to
// either side, 2r + 1 smeared rows are OR-ed: separable, and all in whole words (a word is read by every lane of a row: a broadcast).
constexpr int DIL_HALO = MASK_DILATE_MAX_R, DIL_ROWS = MASK_DILATE_TY + 2 * DIL_HALO;
static_assert(MASK_DILATE_TX + 2 * DIL_HALO == 64, "a window row is one 64-bit word");
__global__ __launch_bounds__(256) void mask_dilate_kernel(const unsigned char *__restrict__ in, int H, int W, int r, unsigned char *__restrict__ out)
{
    __shared__ unsigned long long rows[DIL_ROWS], smeared[DIL_ROWS], col[MASK_DILATE_TY];
    const int t = threadIdx.x, x0 = blockIdx.x * MASK_DILATE_TX, y0 = blockIdx.y * MASK_DILATE_TY;
    for (int q = t; q < DIL_ROWS * 8; q += 256) {
        const int hr = q >> 3, seg = q & 7, y = y0 - DIL_HALO + hr, xs = x0 - DIL_HALO + 8 * seg;
        unsigned bits = 0;
        if (y >= 0 && y < H)
            for (int j = 0; j < 8; j++) {
                const int x = xs + j;
                if (x >= 0 && x < W && in[(long)y * W + x]) bits |= 1u << j;
            }
        ((unsigned char *)rows)[8 * hr + seg] = (unsigned char)bits;  // little endian: bit j of rows[hr] is column x0 - 8 + j
    }
    __syncthreads();
    if (t < DIL_ROWS) {
        const unsigned long long w = rows[t];
        unsigned long long s = w;
        for (int d = 1; d <= r; d++) s |= (w << d) | (w >> d);
        smeared[t] = s;
    }
    __syncthreads();
    if (t < MASK_DILATE_TY) {
        unsigned long long v = 0;
        for (int d = -r; d <= r; d++) v |= smeared[t + DIL_HALO + d];
        col[t] = v;
    }
    __syncthreads();
    for (int o = t; o < MASK_DILATE_TX * MASK_DILATE_TY; o += 256) {
        const int ly = o / MASK_DILATE_TX, lx = o - ly * MASK_DILATE_TX, y = y0 + ly, x = x0 + lx;
        if (y < H && x < W) out[(long)y * W + x] = (unsigned char)((col[ly] >> (lx + DIL_HALO)) & 1ull);
    }
}

// ------------------------------------------------------------------------------------------------
// Constrained propagation, one sweep: sout = sin grown inside every tile to the tile's own fixpoint.  A workgroup is one wave and owns
// MASK_PROPAGATE_T^2 pixels; it reads the 64 x 64 window around them (halo 1), lane = column, one ballot a row, and lane j keeps row j.
// The halo is read, takes part, and is not written.  Every set is a subset of the one fixpoint and sweeps only add, so any schedule ends
// in the same image; the host repeats sweeps while *changed comes back non-zero.  No workgroup waits for another: `changed` is the only
// word two workgroups share, and each stores the same 1 into it.
static_assert(MASK_PROPAGATE_T + 2 == 64, "a window row is one 64-bit word, a window one wave of rows");
__global__ __launch_bounds__(64) void mask_propagate_kernel(const unsigned char *__restrict__ sin, const unsigned char *__restrict__ grow, int H, int W,
                                                            unsigned char *__restrict__ sout, unsigned int *__restrict__ changed)
{
    __shared__ unsigned long long S[64 + 2];  // row j at S[j + 1]; S[0] and S[65] stay 0
    const int t = threadIdx.x, x0 = blockIdx.x * MASK_PROPAGATE_T, y0 = blockIdx.y * MASK_PROPAGATE_T;
    const int x = x0 - 1 + t;
    unsigned long long s = 0, g = 0;
    for (int j = 0; j < 64; j++) {
        const int y = y0 - 1 + j;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const unsigned long long ws = __ballot(in && sin[(long)y * W + x] != 0), wg = __ballot(in && grow[(long)y * W + x] != 0);
        if (j == t) s = ws, g = wg;
    }
    const unsigned long long s_in = s;
    S[t + 1] = s;
    if (t == 0) S[0] = 0, S[65] = 0;
    __syncthreads();
    for (int it = 0; it < 64 * 64; it++) {  // (every round but the last sets a pixel of the window)
        const unsigned long long n = om_flood_row(s, S[t], S[t + 2], g);
        const bool moved = n != s;
        __syncthreads();
        if (moved) S[t + 1] = s = n;
        if (!__syncthreads_or(moved ? 1 : 0)) break;
    }
    for (int j = 1; j <= MASK_PROPAGATE_T; j++) {
        const int y = y0 - 1 + j;
        if (y < H && t >= 1 && t <= MASK_PROPAGATE_T && x < W) sout[(long)y * W + x] = (unsigned char)((S[j + 1] >> t) & 1ull);
    }
    const bool mine = t >= 1 && t <= MASK_PROPAGATE_T && ((s ^ s_in) & 0x7FFFFFFFFFFFFFFEull) != 0;  // (pixels beyond H or W have no grow bit: never set)
    if (__syncthreads_or(mine ? 1 : 0) && t == 0) *changed = 1u;
}

// ------------------------------------------------------------------------------------------------
template <typename T>
static int select_kth_t(imcom_ctx *ctx, const T *vals, const unsigned char *flags, long n, bool use_abs, double c, long k, unsigned long long *state,
                        unsigned long long *hist, void *res, long *info)
{
    const int keybits = 8 * (int)sizeof(T), blocks = (int)std::min<long>((n + 255) / 256, 4L * ctx->cu_count);
    for (int pass = 0; pass < om_passes(keybits); pass++) {
        hipLaunchKernelGGL(select_hist_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, vals, flags, n, use_abs ? 1 : 0, (T)c, pass, state, hist);
        IMCOM_TRY(check_launch("select_hist_kernel"));
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, ctx->stream, keybits == 64 ? 1 : 0, pass, k, state, hist, res, info);
        IMCOM_TRY(check_launch("select_pick_kernel"));
    }
    return IMCOM_OK;
}

static int launch_select_kth(imcom_ctx *ctx, const void *vals, bool f64, const unsigned char *flags, long n, bool use_abs, double c, long k, unsigned long long *state,
                      unsigned long long *hist, void *res, long *info)
{
    ProfScope ps(ctx, "select_kth");
    IMCOM_HIP_CHECK(hipMemsetAsync(state, 0, SELECT_STATE * sizeof(unsigned long long), ctx->stream));
    IMCOM_HIP_CHECK(hipMemsetAsync(hist, 0, 2 * SELECT_BINS * sizeof(unsigned long long), ctx->stream));
    static_assert(SELECT_BINS == OM_BINS, "the histogram the entry reserves");
    return f64 ? select_kth_t(ctx, (const double *)vals, flags, n, use_abs, c, k, state, hist, res, info)
               : select_kth_t(ctx, (const float *)vals, flags, n, use_abs, c, k, state, hist, res, info);
}

static unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

static int launch_mask_threshold(imcom_ctx *ctx, const void *img, bool f64, long n, double bkg, double t1, double t2, bool finite_only, unsigned char *m1,
                          unsigned char *m2)
{
    ProfScope ps(ctx, "mask_flags");
    if (f64) hipLaunchKernelGGL(mask_threshold_kernel<double>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const double *)img, n, bkg, t1, t2, finite_only ? 1 : 0, m1, m2);
    else hipLaunchKernelGGL(mask_threshold_kernel<float>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const float *)img, n, (float)bkg, t1, t2, finite_only ? 1 : 0, m1, m2);
    return check_launch("mask_threshold_kernel");
}

static int launch_mask_clip(imcom_ctx *ctx, const void *img, bool f64, long n, const unsigned char *keep_in, double bkg, double t, unsigned char *keep_out,
                     unsigned long long *count)
{
    ProfScope ps(ctx, "mask_flags");
    IMCOM_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), ctx->stream));
    if (f64) hipLaunchKernelGGL(mask_clip_kernel<double>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const double *)img, n, keep_in, bkg, t, keep_out, count);
    else hipLaunchKernelGGL(mask_clip_kernel<float>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const float *)img, n, keep_in, (float)bkg, t, keep_out, count);
    return check_launch("mask_clip_kernel");
}

static int launch_mask_apply(imcom_ctx *ctx, const void *in, int dtype, const unsigned char *mask, long n, void *out)
{
    ProfScope ps(ctx, "mask_apply");
    if (dtype == 1) hipLaunchKernelGGL(mask_apply_kernel<double>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const double *)in, mask, n, (double *)out);
    else if (dtype == 0) hipLaunchKernelGGL(mask_apply_kernel<float>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const float *)in, mask, n, (float *)out);
    else hipLaunchKernelGGL(mask_apply_kernel<unsigned char>, dim3(blocks_of(n)), dim3(256), 0, ctx->stream, (const unsigned char *)in, mask, n, (unsigned char *)out);
    return check_launch("mask_apply_kernel");
}

static int launch_mask_dilate(imcom_ctx *ctx, const unsigned char *in, int H, int W, int r, unsigned char *out)
{
    ProfScope ps(ctx, "mask_dilate");
    hipLaunchKernelGGL(mask_dilate_kernel, dim3((unsigned)((W + MASK_DILATE_TX - 1) / MASK_DILATE_TX), (unsigned)((H + MASK_DILATE_TY - 1) / MASK_DILATE_TY)), dim3(256),
                       0, ctx->stream, in, H, W, r, out);
    return check_launch("mask_dilate_kernel");
}

// out (already holding the seed) to the fixpoint; tmp: a second image.  Sweeps go in pairs, out -> tmp -> out, so the result is always in
// `out`; a pair that changes nothing ends the loop (then out == tmp == the fixpoint).  A sweep that changes something sets at least one
// pixel: H W / 2 + 1 pairs bound the loop.
static int launch_mask_propagate(imcom_ctx *ctx, const unsigned char *grow, int H, int W, unsigned char *out, unsigned char *tmp, unsigned int *changed, long *sweeps)
{
    ProfScope ps(ctx, "mask_propagate");
    const dim3 grid((unsigned)((W + MASK_PROPAGATE_T - 1) / MASK_PROPAGATE_T), (unsigned)((H + MASK_PROPAGATE_T - 1) / MASK_PROPAGATE_T));
    const long max_pairs = (long)H * W / 2 + 1;
    *sweeps = 0;
    for (long pair = 0; pair < max_pairs; pair++) {
        unsigned int moved = 0;
        IMCOM_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(unsigned int), ctx->stream));
        hipLaunchKernelGGL(mask_propagate_kernel, grid, dim3(64), 0, ctx->stream, (const unsigned char *)out, grow, H, W, tmp, changed);
        IMCOM_TRY(check_launch("mask_propagate_kernel"));
        hipLaunchKernelGGL(mask_propagate_kernel, grid, dim3(64), 0, ctx->stream, (const unsigned char *)tmp, grow, H, W, out, changed);
        IMCOM_TRY(check_launch("mask_propagate_kernel"));
        IMCOM_HIP_CHECK(hipMemcpyAsync(&moved, changed, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *sweeps += 2;
        if (!moved) return IMCOM_OK;
    }
    set_error("mask_propagate: no fixpoint after %ld sweeps of %d x %d pixels", *sweeps, H, W);
    return IMCOM_ERR_HIP;
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: Bright-object masks of the destripe set-up

namespace {
constexpr long MASK_MAX_SIDE = 65536;
}

extern "C" {

int imcom_select_kth(imcom_ctx *ctx, const void *values, int is_f64, long n, const unsigned char *flags, int use_abs, double c, long k, void *out, long *info,
                     int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(values && out && info, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "select_kth: n = %ld outside 1 .. 2^32", n);
    IMCOM_REQUIRE(k < n, "select_kth: rank %ld of %ld values", k, n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add(SELECT_STATE * sizeof(unsigned long long));
    plan.add(2 * SELECT_BINS * sizeof(unsigned long long));
    st.plan(plan, {(size_t)n * esz, flags ? (size_t)n : 0, 2 * esz, 2 * sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *state, *hist;
    const char *v_d;
    const unsigned char *f_d;
    char *o_d;
    long *i_d;
    IMCOM_TRY(ws_take(ctx, (size_t)SELECT_STATE, &state, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)2 * SELECT_BINS, &hist, __func__));
    IMCOM_TRY(st.in((const char *)values, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.in(flags, (size_t)n, &f_d));
    IMCOM_TRY(st.out((char *)out, 2 * esz, &o_d));
    IMCOM_TRY(st.out(info, (size_t)2, &i_d));
    IMCOM_TRY(launch_select_kth(ctx, v_d, is_f64 != 0, f_d, n, use_abs != 0, c, k, state, hist, o_d, i_d));
    IMCOM_TRY(st.back((char *)out, (const char *)o_d, 2 * esz));
    IMCOM_TRY(st.back(info, (const long *)i_d, (size_t)2));
    return st.done();
}

int imcom_mask_threshold(imcom_ctx *ctx, const void *image, int is_f64, long n, double bkg, double t_seed, double t_grow, int finite_only, unsigned char *seed,
                         unsigned char *grow, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && seed, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_threshold: n = %ld outside 1 .. 2^32", n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, (size_t)n, grow ? (size_t)n : 0});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d;
    unsigned char *s_d, *g_d = nullptr;
    IMCOM_TRY(st.in((const char *)image, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.out(seed, (size_t)n, &s_d));
    if (grow) IMCOM_TRY(st.out(grow, (size_t)n, &g_d));
    IMCOM_TRY(launch_mask_threshold(ctx, v_d, is_f64 != 0, n, bkg, t_seed, t_grow, finite_only != 0, s_d, g_d));
    IMCOM_TRY(st.back(seed, (const unsigned char *)s_d, (size_t)n));
    if (grow) IMCOM_TRY(st.back(grow, (const unsigned char *)g_d, (size_t)n));
    return st.done();
}

int imcom_mask_clip(imcom_ctx *ctx, const void *image, int is_f64, long n, const unsigned char *keep_in, double bkg, double t, unsigned char *keep_out, long *count,
                    int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && keep_out && count, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_clip: n = %ld outside 1 .. 2^32", n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, keep_in ? (size_t)n : 0, (size_t)n, sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d;
    const unsigned char *ki_d;
    unsigned char *ko_d;
    long *c_d;
    IMCOM_TRY(st.in((const char *)image, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.in(keep_in, (size_t)n, &ki_d));
    IMCOM_TRY(st.out(keep_out, (size_t)n, &ko_d));
    IMCOM_TRY(st.out(count, (size_t)1, &c_d));
    IMCOM_TRY(launch_mask_clip(ctx, v_d, is_f64 != 0, n, ki_d, bkg, t, ko_d, (unsigned long long *)c_d));
    IMCOM_TRY(st.back(keep_out, (const unsigned char *)ko_d, (size_t)n));
    IMCOM_TRY(st.back(count, (const long *)c_d, (size_t)1));
    return st.done();
}

int imcom_mask_propagate(imcom_ctx *ctx, const unsigned char *seed, const unsigned char *grow, int rows, int cols, unsigned char *out, long *sweeps, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(seed && grow && out, "null pointer");
    IMCOM_REQUIRE(rows >= 1 && rows <= MASK_MAX_SIDE && cols >= 1 && cols <= MASK_MAX_SIDE, "mask_propagate: %d x %d pixels, sides 1 .. 65536", rows, cols);
    IMCOM_REQUIRE(out != grow, "mask_propagate: the result cannot overwrite the grow image");
    const size_t npix = (size_t)rows * cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add(npix);
    plan.add(sizeof(unsigned int));
    st.plan(plan, {npix, npix, npix});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned char *tmp, *o_d;
    unsigned int *changed;
    const unsigned char *s_d, *g_d;
    IMCOM_TRY(ws_take(ctx, npix, &tmp, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)1, &changed, __func__));
    IMCOM_TRY(st.in(seed, npix, &s_d));
    IMCOM_TRY(st.in(grow, npix, &g_d));
    IMCOM_TRY(st.out(out, npix, &o_d));
    if (o_d != s_d) IMCOM_HIP_CHECK(hipMemcpyAsync(o_d, s_d, npix, hipMemcpyDeviceToDevice, ctx->stream));
    long n_sweeps = 0;
    IMCOM_TRY(launch_mask_propagate(ctx, g_d, rows, cols, o_d, tmp, changed, &n_sweeps));
    if (sweeps) *sweeps = n_sweeps;
    IMCOM_TRY(st.back(out, (const unsigned char *)o_d, npix));
    return st.done();
}

int imcom_mask_dilate(imcom_ctx *ctx, const unsigned char *in, int rows, int cols, int r, unsigned char *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(in && out, "null pointer");
    IMCOM_REQUIRE(rows >= 1 && rows <= MASK_MAX_SIDE && cols >= 1 && cols <= MASK_MAX_SIDE, "mask_dilate: %d x %d pixels, sides 1 .. 65536", rows, cols);
    IMCOM_REQUIRE(in != out, "mask_dilate: not in place");
    if (r < 1 || r > MASK_DILATE_MAX_R) {
        set_error("mask_dilate: radius %d, served are 1 .. %d", r, MASK_DILATE_MAX_R);
        return IMCOM_ERR_UNSUPPORTED;
    }
    const size_t npix = (size_t)rows * cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {npix, npix});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned char *i_d;
    unsigned char *o_d;
    IMCOM_TRY(st.in(in, npix, &i_d));
    IMCOM_TRY(st.out(out, npix, &o_d));
    IMCOM_TRY(launch_mask_dilate(ctx, i_d, rows, cols, r, o_d));
    IMCOM_TRY(st.back(out, (const unsigned char *)o_d, npix));
    return st.done();
}

int imcom_mask_apply(imcom_ctx *ctx, const void *in, int dtype, const unsigned char *mask, long n, void *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(in && mask && out, "null pointer");
    IMCOM_REQUIRE(dtype >= 0 && dtype <= 2, "mask_apply: dtype %d is none of 0 (float32), 1 (float64), 2 (uint8)", dtype);
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_apply: n = %ld outside 1 .. 2^32", n);
    const size_t esz = dtype == 0 ? 4 : dtype == 1 ? 8 : 1;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, (size_t)n, (size_t)n * esz});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *i_d;
    const unsigned char *m_d;
    char *o_d;
    IMCOM_TRY(st.in((const char *)in, (size_t)n * esz, &i_d));
    IMCOM_TRY(st.in(mask, (size_t)n, &m_d));
    IMCOM_TRY(st.out((char *)out, (size_t)n * esz, &o_d));
    IMCOM_TRY(launch_mask_apply(ctx, i_d, dtype, m_d, n, o_d));
    IMCOM_TRY(st.back((char *)out, (const char *)o_d, (size_t)n * esz));
    return st.done();
}

}  // extern "C"
