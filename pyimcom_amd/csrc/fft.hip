// fft.hip -- the host side of the line-transform engine that psf_overlap.hip, splitpsf.hip, noisespec.hip and noise1f.hip share (no C entries):
// for the wave-per-line butterflies (fft_lines.h, planned by fft_plan_core.h) the stage tables of a plan and a line kernel's opt-in to the
// dynamic LDS its plan asks for; and the dense-DFT line engine, the fallback of splitpsf.hip and noisespec.hip for the sides the butterflies
// do not take: contiguous complex lines [N] as real rows [2N] times a real [2N x 2N] matrix of 2 x 2 rotation blocks, ONE product on the
// fp64 MFMA tile engine (gemm_f64.hip).
#include <algorithm>

#include "common.h"
#include "fft_lines.h"
#include "launchers.h"

namespace imcom {

__global__ void fft_twiddle_kernel(FftPlan pl, cplx *__restrict__ tw)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= pl.twn) return;
    int s = 1, Ns = pl.radix[0];
    while (s + 1 < pl.nst && e >= pl.twoff[s + 1]) { Ns *= pl.radix[s]; s++; }
    const int local = e - pl.twoff[s], t = local / Ns + 1, k = local - (t - 1) * Ns;
    double c, sn;
    twiddle((long)t * k * (pl.n / (Ns * pl.radix[s])), pl.n, &c, &sn);
    tw[e] = make_double2(c, -sn);
}

int fft_line_twiddles(imcom_ctx *ctx, const FftPlan &pl, cplx *tw)
{
    hipLaunchKernelGGL(fft_twiddle_kernel, dim3((pl.twn + 255) / 256), dim3(256), 0, ctx->stream, pl, tw);
    return check_launch("fft_twiddle_kernel");
}

int fft_line_lds_opt_in(const void *kernel, size_t lds_bytes)
{
    if (lds_bytes > 48 * 1024) IMCOM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return IMCOM_OK;
}

// the dense-DFT line engine: the [Kp x Np] real matrix of the DFT of interleaved complex rows: element x (re, im) to element k (re, im) by the rotation
// (a + i b)(c -+ i s) = (a c +- b s) + i (b c -+ a s), c + i s = exp(2 pi i x k / N); zero outside 2N x 2N
__global__ void dft_dense_matrix_kernel(int N, int Kp, int Np, int inv, double *__restrict__ M)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= Np || i >= Kp) return;
    double v = 0.0;
    if (i < 2 * N && j < 2 * N) {
        double c, s;
        twiddle((long)(i >> 1) * (j >> 1), N, &c, &s);
        if (inv) s = -s;
        v = ((i & 1) == (j & 1)) ? c : ((i & 1) ? s : -s);
    }
    M[(long)i * Np + j] = v;
}

// rows of interleaved complex lines [nlines][2N] -> [Mp][Kp], zero padded
__global__ void dft_dense_pack_kernel(const double *__restrict__ in, long nlines, long Mp, int N2, int Kp, double *__restrict__ A)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const long r = blockIdx.y + (long)blockIdx.z * 65535;
    if (c >= Kp || r >= Mp) return;
    A[r * Kp + c] = (r < nlines && c < N2) ? in[r * N2 + c] : 0.0;
}

void dft_dense_plan(DftDense &d, int N, long nlines, bool inverse, WsPlan &plan)
{
    d.N = N;
    d.Kp = (int)align_up(2 * N, 16);
    d.Np = (int)align_up(2 * N, NB);
    d.Mp = (nlines + NB - 1) / NB * NB;
    plan.add((size_t)d.Kp * d.Np * 8);
    if (inverse) plan.add((size_t)d.Kp * d.Np * 8);
    plan.add((size_t)d.Mp * d.Kp * 8);
    plan.add((size_t)d.Mp * d.Np * 8);
}

int dft_dense_take(imcom_ctx *ctx, DftDense &d, bool inverse, const char *who)
{
    IMCOM_TRY(ws_take(ctx, (size_t)d.Kp * d.Np, &d.Mf, who));
    if (inverse) IMCOM_TRY(ws_take(ctx, (size_t)d.Kp * d.Np, &d.Mi, who));
    IMCOM_TRY(ws_take(ctx, (size_t)d.Mp * d.Kp, &d.A, who));
    IMCOM_TRY(ws_take(ctx, (size_t)d.Mp * d.Np, &d.C, who));
    hipLaunchKernelGGL(dft_dense_matrix_kernel, dim3((d.Np + 255) / 256, d.Kp), dim3(256), 0, ctx->stream, d.N, d.Kp, d.Np, 0, d.Mf);
    if (inverse) hipLaunchKernelGGL(dft_dense_matrix_kernel, dim3((d.Np + 255) / 256, d.Kp), dim3(256), 0, ctx->stream, d.N, d.Kp, d.Np, 1, d.Mi);
    return check_launch("dft_dense_matrix_kernel");
}

int dft_dense_product(imcom_ctx *ctx, const DftDense &d, const cplx *in, long nlines, bool inv)
{
    const long Mp = (nlines + NB - 1) / NB * NB;
    IMCOM_REQUIRE(Mp <= d.Mp && Mp <= 0x7fffffffL && (!inv || d.Mi), "internal: dense DFT batch of %ld lines", nlines);
    hipLaunchKernelGGL(dft_dense_pack_kernel, dim3((d.Kp + 255) / 256, (unsigned)std::min<long>(Mp, 65535), (unsigned)((Mp + 65534) / 65535)), dim3(256), 0,
                       ctx->stream, (const double *)in, nlines, Mp, 2 * d.N, d.Kp, d.A);
    IMCOM_TRY(check_launch("dft_dense_pack_kernel"));
    return launch_gemm(ctx, false, true, (int)Mp, d.Np, d.Kp, 1, d.A, d.Kp, 0, inv ? d.Mi : d.Mf, d.Np, 0, d.C, d.Np, 0, 1.0, 0.0);
}

}  // namespace imcom
