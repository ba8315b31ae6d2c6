// noise1f.hip -- the transform of the 1/f noise layer (reference src/pyimcom/layer.py:896-913, the channel loop of CplxNoise.noise_1f_frame).
//
// Per channel c the reference forms x[n] = (g[2c][n] + i g[2c+1][n]) amp[n] from 2 len normal draws, takes the forward DFT of length len,
// keeps the real part of outputs k < len / 2, divides by sqrt(2), subtracts the mean and lays the [len / 2 / w][w] block into columns
// c w .. c w + w - 1 of a float32 frame, odd channels with their columns reversed; the frame is returned without a border of 4 pixels.
//
// The DFT is a four-step transform on the wave-per-line butterflies of fft_lines.h (their plans: fft_plan_core.h, their stage tables: fft.hip):
// len = N1 N2 (powers of two, 32 .. 1024 each; N1 >= N2), n = n1 N2 + n2, k = k1 + N1 k2:
//   step 1  for every n2 the DFT over n1 of x[n1 N2 + n2] (amp applied in the loads), times exp(-2 pi i n2 k1 / len) in the stores (the
//           twiddle from cospi / sinpi of the exactly reduced angle) -> S[c][n2][k1]
//   step 2  for every k1 the DFT over n2 of S[c][.][k1]; only k2 < N2 / 2 is stored, and only its real part: blk[c][k1 + N1 k2] = Re / sqrt(2)
// then the channel sum in a fixed order (a thread's elements in ascending order, then a tree over the threads), and one pass that
// subtracts the mean in float64, and casts and places the pixel.  Every element has one owner thread; nothing depends on the launch shape.
#include <algorithm>

#include "common.h"
#include "fft_lines.h"
#include "launchers.h"

namespace imcom {

// line L = (channel c of the group, n2): g, S and nlines are the group's
__global__ __launch_bounds__(WF_MAXWAVES * 64) void n1f_step1_kernel(const double *__restrict__ g, const double *__restrict__ amp, int len, int N2, long nlines,
                                                                     FftPlan pl, const cplx *__restrict__ tw, cplx *__restrict__ S)
{
    const WfWave w = wf_prologue(pl, tw, pl.waves);
    const long L = (long)blockIdx.x * pl.waves + w.wave;
    if (L >= nlines) return;  // (no workgroup barrier below)
    const long c = L / N2;
    const int n2 = (int)(L - c * N2);
    const double *re = g + 2 * c * len + n2, *im = re + len, *a = amp + n2;
    cplx *dst = S + L * pl.n;
    auto load0 = [&](int n1) {
        const long o = (long)n1 * N2;
        const double w = a[o];
        return make_double2(re[o] * w, im[o] * w);
    };
    auto storeN = [&](int k1, cplx v) {
        double cs, sn;
        twiddle((long)n2 * k1, len, &cs, &sn);
        dst[k1] = cmulf(v, make_double2(cs, -sn));
    };
    wf_line<false>(w.line, w.twl, pl, load0, storeN);
}

// line L = (channel c of the group, k1); pl.n = N2
__global__ __launch_bounds__(WF_MAXWAVES * 64) void n1f_step2_kernel(const cplx *__restrict__ S, int N1, long nlines, FftPlan pl, const cplx *__restrict__ tw,
                                                                     double *__restrict__ blk)
{
    const WfWave w = wf_prologue(pl, tw, pl.waves);
    const long L = (long)blockIdx.x * pl.waves + w.wave;
    if (L >= nlines) return;  // (no workgroup barrier below)
    const long c = L / N1;
    const int k1 = (int)(L - c * N1), N2 = pl.n;
    const cplx *src = S + c * N1 * N2 + k1;
    double *dst = blk + c * (N1 * (long)N2 / 2) + k1;
    auto load0 = [&](int n2) { return src[(long)n2 * N1]; };
    auto storeN = [&](int k2, cplx v) {
        if (2 * k2 < N2) dst[(long)k2 * N1] = v.x / 1.4142135623730951;
    };
    wf_line<false>(w.line, w.twl, pl, load0, storeN);
}

// sum[c] of blk[c][0 .. half): thread t adds elements t, t + 1024, ... in ascending order, then a tree over the 1024 threads
__global__ __launch_bounds__(1024) void n1f_sum_kernel(const double *__restrict__ blk, long half, double *__restrict__ sum)
{
    __shared__ double part[1024];
    const double *b = blk + blockIdx.x * half;
    double s = 0.0;
    for (long i = threadIdx.x; i < half; i += 1024) s += b[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) sum[blockIdx.x] = part[0];
}

// element i of channel c: minus the mean (kept in blk), and as float32 into pixel (i / w, c w + i % w, reversed in odd channels) of the
// frame, of which the rows and columns border .. side - border - 1 are stored
__global__ void n1f_place_kernel(double *__restrict__ blk, const double *__restrict__ sum, long half, int w, int nch, int border, float *__restrict__ frame)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= half) return;
    const double v = blk[c * half + i] - sum[c] / (double)half;
    blk[c * half + i] = v;
    const long rows = half / w, cols = (long)nch * w, y = i / w - border;
    const int xin = (int)(i % w);
    const long x = (long)c * w + ((c & 1) ? w - 1 - xin : xin) - border;
    if (y >= 0 && y < rows - 2 * border && x >= 0 && x < cols - 2 * border) frame[y * (cols - 2 * border) + x] = (float)v;
}

// len = N1 N2 for the four-step transform, false if len is no power of two in 2^10 .. 2^20
static bool noise1f_split(long len, int *N1, int *N2)
{
    if (len < 1024 || len > (1L << 20) || (len & (len - 1))) return false;
    int lg = 0;
    while ((1L << lg) < len) lg++;
    *N2 = 1 << (lg / 2);
    *N1 = (int)(len / *N2);
    return true;
}

// the stage tables of the two line plans: tw1 [N1], tw2 [N2] complex values
static int noise1f_tables(imcom_ctx *ctx, long len, cplx *tw1, cplx *tw2)
{
    int N1, N2;
    FftPlan p1, p2;
    IMCOM_REQUIRE(noise1f_split(len, &N1, &N2) && fft_line_plan(N1, &p1) && fft_line_plan(N2, &p2), "internal: noise_1f length %ld", len);
    IMCOM_TRY(fft_line_twiddles(ctx, p1, tw1));
    return fft_line_twiddles(ctx, p2, tw2);
}

// the channels ch0 .. ch0 + nchg - 1: g [2 nch][len] and blk [nch][len / 2] are the whole call's, S [nchg][len] the group's scratch; tw1 /
// tw2: the stage tables of the N1 / N2 plans
static int launch_noise1f_group(imcom_ctx *ctx, const double *g, const double *amp, long len, int ch0, int nchg, const cplx *tw1, const cplx *tw2, cplx *S, double *blk)
{
    int N1, N2;
    FftPlan p1, p2;
    IMCOM_REQUIRE(noise1f_split(len, &N1, &N2) && fft_line_plan(N1, &p1) && fft_line_plan(N2, &p2), "internal: noise_1f length %ld", len);
    const size_t l1 = fft_line_lds_bytes(p1), l2 = fft_line_lds_bytes(p2);
    IMCOM_TRY(fft_line_lds_opt_in((const void *)n1f_step1_kernel, l1));
    IMCOM_TRY(fft_line_lds_opt_in((const void *)n1f_step2_kernel, l2));
    const long lines1 = (long)nchg * N2, lines2 = (long)nchg * N1;
    ProfScope ps(ctx, "n1f_transform", 2);
    hipLaunchKernelGGL(n1f_step1_kernel, dim3((unsigned)((lines1 + p1.waves - 1) / p1.waves)), dim3(64 * p1.waves), l1, ctx->stream, g + 2L * ch0 * len, amp, (int)len,
                       N2, lines1, p1, tw1, S);
    IMCOM_TRY(check_launch("n1f_step1_kernel"));
    hipLaunchKernelGGL(n1f_step2_kernel, dim3((unsigned)((lines2 + p2.waves - 1) / p2.waves)), dim3(64 * p2.waves), l2, ctx->stream, (const cplx *)S, N1, lines2, p2,
                       tw2, blk + (long)ch0 * (len / 2));
    return check_launch("n1f_step2_kernel");
}

// the channel sums (sum [nch]), blk minus its channel mean in place, and the float32 frame without its border
static int launch_noise1f_place(imcom_ctx *ctx, double *blk, double *sum, long len, int nch, int w, int border, float *frame)
{
    const long half = len / 2;
    ProfScope ps(ctx, "n1f_place", 2);
    hipLaunchKernelGGL(n1f_sum_kernel, dim3(nch), dim3(1024), 0, ctx->stream, (const double *)blk, half, sum);
    IMCOM_TRY(check_launch("n1f_sum_kernel"));
    hipLaunchKernelGGL(n1f_place_kernel, dim3((unsigned)((half + 255) / 256), nch), dim3(256), 0, ctx->stream, blk, (const double *)sum, half, w, nch, border, frame);
    return check_launch("n1f_place_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: The transform of the 1/f noise layer

constexpr int NOISE1F_GROUP = 8;  // channels that share one pass (and the scratch S: 128 MB at len = 2^20)

extern "C" {

int imcom_noise_1f(imcom_ctx *ctx, const double *normals, const double *amp, long len, int nch, int w, int border, float *frame, double *block, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(len >= 2 && nch >= 1 && nch <= 4096 && w >= 1 && border >= 0, "noise_1f: len %ld, %d channels of width %d, border %d", len, nch, w, border);
    int N1, N2;
    if ((w & (w - 1)) || !noise1f_split(len, &N1, &N2) || (long)w > len / 2) {
        set_error("noise_1f: the length (%ld) must be a power of two in 2^10 .. 2^20 and the channel width (%d) a power of two up to half of it", len, w);
        return IMCOM_ERR_UNSUPPORTED;
    }
    IMCOM_REQUIRE(normals && amp && frame, "null pointer");
    const long half = len / 2, rows = half / w, cols = (long)nch * w;
    IMCOM_REQUIRE(2L * border < rows && 2L * border < cols, "noise_1f: a border of %d leaves nothing of %ld x %ld pixels", border, rows, cols);
    const long npix = (rows - 2 * border) * (cols - 2 * border);
    const int group = std::min(nch, NOISE1F_GROUP);
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)N1 * 16);
    plan.add((size_t)N2 * 16);
    plan.add((size_t)group * len * 16);  // S
    plan.add((size_t)nch * 8);           // sums
    if (st.host || !block) plan.add((size_t)nch * half * 8);
    st.plan(plan, {(size_t)2 * nch * len * 8, (size_t)len * 8, (size_t)npix * 4});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    double2 *tw1, *tw2, *S;
    double *sum, *blk = block;
    const double *g_d, *amp_d;
    float *f_d;
    IMCOM_TRY(ws_take(ctx, (size_t)N1, &tw1, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)N2, &tw2, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)group * len, &S, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)nch, &sum, __func__));
    if (st.host || !block) IMCOM_TRY(ws_take(ctx, (size_t)nch * half, &blk, __func__));
    IMCOM_TRY(st.in(normals, (size_t)2 * nch * len, &g_d));
    IMCOM_TRY(st.in(amp, (size_t)len, &amp_d));
    IMCOM_TRY(st.out(frame, (size_t)npix, &f_d));
    IMCOM_TRY(noise1f_tables(ctx, len, tw1, tw2));
    for (int ch0 = 0; ch0 < nch; ch0 += group)
        IMCOM_TRY(launch_noise1f_group(ctx, g_d, amp_d, len, ch0, std::min(group, nch - ch0), tw1, tw2, S, blk));
    IMCOM_TRY(launch_noise1f_place(ctx, blk, sum, len, nch, w, border, f_d));
    IMCOM_TRY(st.back(frame, (const float *)f_d, (size_t)npix));
    if (block) IMCOM_TRY(st.back(block, (const double *)blk, (size_t)nch * half));
    return st.done();
}

}  // extern "C"
