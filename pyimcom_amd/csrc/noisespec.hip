// noisespec.hip -- noise power spectra of coadded frames on the device.
//
// Replaces the numerical content of NoiseAnal.__call__ (reference src/pyimcom/analysis.py:745-807: rfft2, |F|^2 / norm, the fold to the
// shifted full spectrum 790-793, the 8 x 8 averages 794, the azimuthal average 661-704), of the accumulation loop of
// _BlkGrp.get_noise_power_spectra (1270-1292) and of NoiseReport.measure_power_spectrum / azimuthal_average
// (diagnostics/noise_diagnostics.py:400-443, 472-506: the Tukey window handed in by the caller, fft2, 8 x 8 averages).
//
// The real 2-D transform of a frame [L][L] (L even) in float64, whatever the input type:
//   row pass     rows 2j, 2j+1 ride as ONE complex line z = a + i b; after its transform Z the two spectra are separated,
//                A_k = (Z_k + conj Z_-k) / 2, B_k = (Z_k - conj Z_-k) / 2i, k <= L/2, and stored transposed: H[frame][k][row];
//   column pass  the L/2 + 1 contiguous lines H[frame][k][:] -> F[frame][kx][ky], kx <= L/2 (the half spectrum, x-frequency major).
// Only rows of one frame are paired, so a frame's result depends on that frame alone: the same bits however frames are grouped into calls.
//
// A line of length L = N1 N2 is N2 sub-transforms of length N1 (decimation in time: sub-transform n2 takes elements N2 n1 + n2), each by
// one wave with the butterflies of fft_lines.h, its stages exchanged in place in the wave's own N1-element region of LDS; then, per k1,
// the twiddles w_L^(n2 k1) and a direct DFT of length N2 <= 16 (in place again: a thread owns the column k1 of the N2 regions):
// X[k1 + N1 k2] = sum_n2 w_N2^(n2 k2) w_L^(n2 k1) Y_n2[k1].  A workgroup owns G lines:
//   route "lines"      N2 = 1, L a side fft_line_plan takes, G = the plan's waves per workgroup;
//   route "two-level"  2 <= N2 <= 16, the smallest N2 for which N1 = L / N2 is a side the butterflies take (a fft_line_plan side, or 4, 8, 16
//                      as two stages: fft_short_plan; both in fft_plan_core.h), G = 1: 2560 = 640 x 4, 2688 = 384 x 7, 1040 = 80 x 13, 56 = 8 x 7.
//                      LDS: L complex128 values + the stage tables (< N1 values): 50 KB at 2560, 48 KB at 2688, 68 KB at 4096 = 1024 x 4;
//   route "dense"      every other side: the dense-DFT line engine of fft.hip (fp64 MFMA tiles), with pack / unpack kernels around it.
//
// Determinism: every output element of every kernel has one owner thread and a fixed summation order; no atomics anywhere.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "fft_lines.h"
#include "launchers.h"

namespace imcom {

constexpr int NOISEPS_ROUTE_NONE = 0, NOISEPS_ROUTE_LINES = 1, NOISEPS_ROUTE_DENSE = 2, NOISEPS_ROUTE_TWOLEVEL = 3;
constexpr int NS_MAXN2 = 16;
constexpr int NS_MAXWAVES = 8;  // waves per workgroup: two per SIMD leave a wave 256 registers (a radix-16 butterfly with its twiddles needs ~140, the N2 column 64 more)

// L = N1 N2 for the route, pl the plan of the length-N1 sub-transforms: what fft_line_plan takes, or 4, 8, 16 as two stages
// (fft_short_plan); false: dense
static bool ns_factor(int L, FftPlan *pl, int *N2)
{
    if (fft_line_plan(L, pl)) { *N2 = 1; return true; }
    for (int n2 = 2; n2 <= NS_MAXN2; n2++)
        if (L % n2 == 0 && (fft_line_plan(L / n2, pl) || fft_short_plan(L / n2, pl))) { *N2 = n2; return true; }
    return false;
}

// force_dense: IMCOM_NOISEPS_ROUTE=dense (the caller reads the environment)
static int noiseps_route(int L, bool force_dense)
{
    if (L < 2 || L % 2 != 0 || L > DFT_DENSE_MAXN) return NOISEPS_ROUTE_NONE;
    FftPlan pl;
    int N2;
    if (force_dense || !ns_factor(L, &pl, &N2)) return NOISEPS_ROUTE_DENSE;
    return N2 == 1 ? NOISEPS_ROUTE_LINES : NOISEPS_ROUTE_TWOLEVEL;
}

struct NsLines {
    FftPlan pl;        // the sub-transforms (pl.n = N1)
    int L, N2, G;      // line length, sub-transforms per line, lines per workgroup
    long nlines;
    const cplx *tw;    // stage tables of pl (pl.twn values)
    const cplx *twL;   // exp(-2 pi i k / L), k < L (N2 > 1)
    // row pass: the frames, addressed in elements
    const void *in;
    long fstride, rstride;
    const double *win;  // [L][L] or null
    const cplx *lines;  // column pass: [nlines][L]
    cplx *out;
};

static size_t ns_lds_bytes(const NsLines &a) { return fft_line_lds_bytes(a.pl, a.G * a.N2) + NS_MAXN2 * 16; }  // G N2 slices, the tables, the N2 roots

__global__ void ns_twiddle_kernel(int L, cplx *__restrict__ twL)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L) return;
    double c, s;
    twiddle(k, L, &c, &s);
    twL[k] = make_double2(c, -s);
}

// ROWS: line = (frame, row pair j) of the input of type T, separated spectra to H[frame][k][2j], [2j+1];  !ROWS: line of a.lines to a.out
// LOOP: more sub-transforms than waves (N2 > 8), a wave takes several.  The loop costs registers (the compiler keeps every stage's
// addresses live across it and spills), so the sides that matter (N2 <= 8: 2560, 2688, 4096) run the straight version.
template <class T, bool ROWS, bool LOOP>
__global__ __launch_bounds__(NS_MAXWAVES * 64) void ns_lines_kernel(NsLines a)
{
    extern __shared__ cplx fbuf[];
    const FftPlan &pl = a.pl;
    const int N1 = pl.n, npad = pl.npad, N2 = a.N2, G = a.G, L = a.L, half = L / 2;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
    cplx *twl = wf_stage_tables(fbuf, pl, a.tw, G * N2), *wn = twl + pl.twn;  // stage tables, then exp(-2 pi i m / N2)
    if ((int)threadIdx.x < N2) {
        double c, s;
        twiddle(threadIdx.x, N2, &c, &s);
        wn[threadIdx.x] = make_double2(c, -s);
    }
    __syncthreads();
    const long line0 = (long)blockIdx.x * G;
    auto sub = [&](int task) {  // sub-transform n2 of line g, by this wave
        const int g = task / N2, n2 = task - g * N2;
        const long line = line0 + g;
        if (line >= a.nlines) return;
        cplx *reg = fbuf + task * npad;
        // the wave's elements N2 i + n2 into its region first: the butterflies then load from LDS, whatever the source looks like
        if constexpr (ROWS) {
            const long f = line / half;
            const int j = (int)(line - f * half);
            const T *p0 = (const T *)a.in + f * a.fstride + (long)(2 * j) * a.rstride, *p1 = p0 + a.rstride;
            const double *w0 = a.win ? a.win + (long)(2 * j) * L : nullptr;
            for (int i = threadIdx.x & 63; i < N1; i += 64) {
                const int x = i * N2 + n2;
                double re = (double)p0[x], im = (double)p1[x];
                if (w0) re *= w0[x], im *= w0[L + x];
                reg[wf_swz(i)] = make_double2(re, im);
            }
        } else {
            const cplx *src = a.lines + line * L;
            for (int i = threadIdx.x & 63; i < N1; i += 64) reg[wf_swz(i)] = src[i * N2 + n2];
        }
        __builtin_amdgcn_wave_barrier();
        wf_line<false>(reg, twl, pl, [reg](int i) { return reg[wf_swz(i)]; }, [reg](int k, cplx v) { reg[wf_swz(k)] = v; });
    };
    if constexpr (LOOP) {
        for (int task = wave; task < G * N2; task += W) sub(task);
    } else {
        if (wave < G * N2) sub(wave);
    }
    __syncthreads();
    if (N2 > 1) {
        for (int c = threadIdx.x; c < G * N1; c += blockDim.x) {
            const int g = c / N1, k1 = c - g * N1;
            if (line0 + g >= a.nlines) continue;
            cplx *base = fbuf + g * N2 * npad + wf_swz(k1);
            cplx t[NS_MAXN2];
#pragma unroll
            for (int n2 = 0; n2 < NS_MAXN2; n2++)
                if (n2 < N2) {
                    cplx v = base[n2 * npad];
                    if (n2) v = cmulf(v, a.twL[n2 * k1]);
                    t[n2] = v;
                }
            for (int k2 = 0; k2 < N2; k2++) {
                cplx acc = t[0];
                int m = 0;  // n2 k2 mod N2
#pragma unroll
                for (int n2 = 1; n2 < NS_MAXN2; n2++)
                    if (n2 < N2) {
                        m += k2;
                        if (m >= N2) m -= N2;
                        acc = cadd(acc, cmulf(t[n2], wn[m]));
                    }
                base[k2 * npad] = acc;
            }
        }
        __syncthreads();
    }
    // X[k] of line g sits at region k / N1 of the line, element k mod N1
    auto X = [&](int g, int k) {
        const int k2 = k / N1, k1 = k - k2 * N1;
        return fbuf[(g * N2 + k2) * npad + wf_swz(k1)];
    };
    if constexpr (ROWS) {
        const int nh = half + 1;
        for (int c = threadIdx.x; c < G * nh; c += blockDim.x) {  // g fastest: neighbouring row pairs write neighbouring elements
            const int k = c / G, g = c - k * G;
            const long line = line0 + g;
            if (line >= a.nlines) continue;
            const long f = line / half;
            const int j = (int)(line - f * half);
            const cplx z = X(g, k), m = X(g, k == 0 ? 0 : L - k);
            cplx *dst = a.out + (f * nh + k) * L + 2 * j;
            dst[0] = make_double2(0.5 * (z.x + m.x), 0.5 * (z.y - m.y));
            dst[1] = make_double2(0.5 * (z.y + m.y), -0.5 * (z.x - m.x));
        }
    } else {
        for (int c = threadIdx.x; c < G * L; c += blockDim.x) {
            const int g = c / L, k = c - g * L;
            if (line0 + g >= a.nlines) continue;
            a.out[(line0 + g) * L + k] = X(g, k);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// the dense route's kernels around dft_dense_product
template <class T>
__global__ void ns_dense_pack_kernel(const T *__restrict__ in, long fstride, long rstride, const double *__restrict__ win, int L, cplx *__restrict__ Z)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    const long f = blockIdx.z;
    if (x >= L) return;
    const T *p0 = in + f * fstride + (long)(2 * j) * rstride;
    double re = (double)p0[x], im = (double)p0[rstride + x];
    if (win) re *= win[(long)(2 * j) * L + x], im *= win[(long)(2 * j + 1) * L + x];
    Z[(f * (L / 2) + j) * L + x] = make_double2(re, im);
}

// C row (f, j) -> H[f][k][2j], [2j+1]
__global__ void ns_dense_separate_kernel(const double *__restrict__ C, int Np, int L, cplx *__restrict__ H)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y, half = L / 2;
    const long f = blockIdx.z;
    if (j >= half) return;
    const double *row = C + (f * half + j) * Np;
    const int km = k == 0 ? 0 : L - k;
    const cplx z = make_double2(row[2 * k], row[2 * k + 1]), m = make_double2(row[2 * km], row[2 * km + 1]);
    cplx *dst = H + (f * (half + 1) + k) * L + 2 * j;
    dst[0] = make_double2(0.5 * (z.x + m.x), 0.5 * (z.y - m.y));
    dst[1] = make_double2(0.5 * (z.y + m.y), -0.5 * (z.x - m.x));
}

__global__ void ns_dense_copy_kernel(const double *__restrict__ C, int Np, int L, long nlines, cplx *__restrict__ F)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const long l = blockIdx.y + (long)blockIdx.z * 65535;
    if (k >= L || l >= nlines) return;
    F[l * L + k] = make_double2(C[l * Np + 2 * k], C[l * Np + 2 * k + 1]);
}

// ---------------------------------------------------------------------------------------------------------
// the epilogue: ps[ky][kx] = |Full[(ky - L/2) mod L][(kx - L/2) mod L]|^2 / norm from the half spectrum F[kx'][ky'], kx' <= L/2; the
// other half by Hermitian symmetry (analysis.py:790-793).  bin8: the 8 x 8 averages (794), summed in (column, row) order, one division.
__device__ __forceinline__ double ns_power(const cplx *__restrict__ F, int L, int ky, int kx)
{
    const int half = L / 2;
    int fy = ky - half, fx = kx - half;
    if (fy < 0) fy += L;
    if (fx < 0) fx += L;
    if (fx > half) {
        fx = L - fx;
        fy = fy == 0 ? 0 : L - fy;
    }
    const cplx v = F[(long)fx * L + fy];
    return v.x * v.x + v.y * v.y;
}

__global__ void ns_epilogue_kernel(const cplx *__restrict__ F, int L, int bin8, const double *__restrict__ norm, double *__restrict__ out)
{
    const int n = bin8 ? L / 8 : L;
    const int oy = blockIdx.x * blockDim.x + threadIdx.x, ox = blockIdx.y;  // threads along ky: the half spectrum is contiguous in ky
    const long f = blockIdx.z;
    if (oy >= n) return;
    const cplx *Ff = F + f * (long)(L / 2 + 1) * L;
    double v;
    if (bin8) {
        double acc = 0.0;
        for (int dx = 0; dx < 8; dx++)  // (a thread walks the contiguous ky of one kx at a time)
            for (int dy = 0; dy < 8; dy++) acc += ns_power(Ff, L, 8 * oy + dy, 8 * ox + dx) / norm[f];
        v = acc / 64.0;
    } else {
        v = ns_power(Ff, L, oy, ox) / norm[f];
    }
    out[(f * n + oy) * n + ox] = v;
}

// ---------------------------------------------------------------------------------------------------------
// the azimuthal average (analysis.py:699-702, ndimage.mean / standard_deviation / sum over labels): workgroup (index, frame); a thread
// sums its pixels in ascending order, the 256 partial sums go through a fixed tree; two passes (mean, then the squared deviations)
__device__ __forceinline__ double ns_tree(double *red, double v)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void ns_radial_kernel(const double *__restrict__ image, long npix, const int *__restrict__ rbin, int nidx,
                                                        double *__restrict__ mean, double *__restrict__ err)
{
    __shared__ double red[256];
    const int idx = blockIdx.x + 1;
    const long f = blockIdx.y;
    const double *img = image + f * npix;
    double s = 0.0, cnt = 0.0;
    for (long e = threadIdx.x; e < npix; e += 256)
        if (rbin[e] == idx) s += img[e], cnt += 1.0;
    const double total = ns_tree(red, s), np_ = ns_tree(red, cnt), mu = total / np_;  // an empty annulus: 0 / 0 = NaN, as ndimage
    double q = 0.0;
    for (long e = threadIdx.x; e < npix; e += 256)
        if (rbin[e] == idx) {
            const double d = img[e] - mu;
            q += d * d;
        }
    const double ss = ns_tree(red, q);
    if (threadIdx.x == 0) {
        mean[f * nidx + blockIdx.x] = mu;
        err[f * nidx + blockIdx.x] = sqrt(ss / np_) / sqrt(np_);
    }
}

// analysis.py:1278-1279: ps2d_all[layer] += ps2d[layer]; ps1d_all[layer][cbin][r] += (mean, err)[layer][r]
__global__ void ns_accumulate_kernel(const double *__restrict__ ps2d, const double *__restrict__ mean, const double *__restrict__ err, long npix, int nrad, int bins,
                                     int cbin, double *__restrict__ ps2d_all, double *__restrict__ ps1d_all)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long l = blockIdx.y;
    if (e < npix) ps2d_all[l * npix + e] += ps2d[l * npix + e];
    if (e < nrad) {
        double *d = ps1d_all + ((l * bins + cbin) * nrad + e) * 2;
        d[0] += mean[l * nrad + e];
        d[1] += err[l * nrad + e];
    }
}

// ---------------------------------------------------------------------------------------------------------
struct NsPlan {
    int L = 0, nframe = 0, route = 0, N2 = 1;
    FftPlan pl;
    DftDense d;
    long nrow = 0, ncol = 0;  // lines of the two passes
};

static size_t ns_plan(NsPlan &p, int L, int nframe, int route, WsPlan &plan)
{
    p.L = L, p.nframe = nframe, p.route = route;
    p.nrow = (long)nframe * (L / 2), p.ncol = (long)nframe * (L / 2 + 1);
    if (route == NOISEPS_ROUTE_DENSE) {
        dft_dense_plan(p.d, L, p.ncol, false, plan);
    } else {
        ns_factor(L, &p.pl, &p.N2);
        plan.add((size_t)std::max(p.pl.twn, 1) * 16);
        plan.add((size_t)L * 16);
    }
    plan.add((size_t)p.ncol * L * 16);  // H
    plan.add((size_t)p.ncol * L * 16);  // F (the dense route packs its row lines here first)
    return plan.total;
}

static size_t noiseps_ws(int L, int nframe, int route)
{
    NsPlan p;
    WsPlan plan;
    return ns_plan(p, L, nframe, route, plan);
}

template <class T, bool ROWS, bool LOOP> static int ns_launch_lines_as(imcom_ctx *ctx, const NsLines &a)
{
    const size_t lds = ns_lds_bytes(a);
    IMCOM_REQUIRE(lds <= 160 * 1024, "internal: noise spectra line of %d needs %zu bytes of LDS", a.L, lds);
    IMCOM_TRY(fft_line_lds_opt_in((const void *)ns_lines_kernel<T, ROWS, LOOP>, lds));
    const int W = std::min(a.G * a.N2, NS_MAXWAVES);
    hipLaunchKernelGGL((ns_lines_kernel<T, ROWS, LOOP>), dim3((unsigned)((a.nlines + a.G - 1) / a.G)), dim3(64 * W), lds, ctx->stream, a);
    return check_launch("ns_lines_kernel");
}

template <class T, bool ROWS> static int ns_launch_lines(imcom_ctx *ctx, const NsLines &a)
{
    return a.G * a.N2 > NS_MAXWAVES ? ns_launch_lines_as<T, ROWS, true>(ctx, a) : ns_launch_lines_as<T, ROWS, false>(ctx, a);
}

// frames: nframe frames of side L, element (f, y, x) at f fstride + y rstride + x (device memory, float or double); window [L][L] or null;
// norm_dev [nframe]; out [nframe][n][n], n = L / 8 (bin8) or L.  The caller has reserved noiseps_ws(L, nframe, route).
static int launch_noiseps_2d(imcom_ctx *ctx, const void *frames, bool in_f64, int nframe, int L, long fstride, long rstride, const double *window,
                      const double *norm_dev, bool bin8, int route, double *out)
{
    NsPlan p;
    WsPlan plan;
    ns_plan(p, L, nframe, route, plan);
    cplx *tw = nullptr, *twL = nullptr, *H, *F;
    if (route == NOISEPS_ROUTE_DENSE) {
        IMCOM_TRY(dft_dense_take(ctx, p.d, false, __func__));
    } else {
        IMCOM_TRY(ws_take(ctx, (size_t)std::max(p.pl.twn, 1), &tw, __func__));
        IMCOM_TRY(ws_take(ctx, (size_t)L, &twL, __func__));
    }
    IMCOM_TRY(ws_take(ctx, (size_t)p.ncol * L, &H, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)p.ncol * L, &F, __func__));
    hipStream_t st = ctx->stream;
    {
        ProfScope ps(ctx, "noiseps_transform");
        if (route == NOISEPS_ROUTE_DENSE) {
            const dim3 gp((L + 255) / 256, L / 2, nframe);
            if (in_f64) hipLaunchKernelGGL(ns_dense_pack_kernel<double>, gp, dim3(256), 0, st, (const double *)frames, fstride, rstride, window, L, F);
            else hipLaunchKernelGGL(ns_dense_pack_kernel<float>, gp, dim3(256), 0, st, (const float *)frames, fstride, rstride, window, L, F);
            IMCOM_TRY(check_launch("ns_dense_pack_kernel"));
            IMCOM_TRY(dft_dense_product(ctx, p.d, F, p.nrow, false));
            hipLaunchKernelGGL(ns_dense_separate_kernel, dim3((L / 2 + 255) / 256, L / 2 + 1, nframe), dim3(256), 0, st, (const double *)p.d.C, p.d.Np, L, H);
            IMCOM_TRY(check_launch("ns_dense_separate_kernel"));
            IMCOM_TRY(dft_dense_product(ctx, p.d, H, p.ncol, false));
            hipLaunchKernelGGL(ns_dense_copy_kernel, dim3((L + 255) / 256, (unsigned)std::min<long>(p.ncol, 65535), (unsigned)((p.ncol + 65534) / 65535)), dim3(256), 0,
                               st, (const double *)p.d.C, p.d.Np, L, p.ncol, F);
            IMCOM_TRY(check_launch("ns_dense_copy_kernel"));
        } else {
            if (p.pl.twn > 0) IMCOM_TRY(fft_line_twiddles(ctx, p.pl, tw));
            hipLaunchKernelGGL(ns_twiddle_kernel, dim3((L + 255) / 256), dim3(256), 0, st, L, twL);
            IMCOM_TRY(check_launch("ns_twiddle_kernel"));
            NsLines a;
            a.pl = p.pl, a.L = L, a.N2 = p.N2, a.G = p.N2 == 1 ? std::min(p.pl.waves, NS_MAXWAVES) : 1;
            while (a.G > 1 && ns_lds_bytes(a) > 160 * 1024) a.G--;  // (the plan's waves fill LDS without the N2 table)
            a.tw = tw, a.twL = twL, a.in = frames, a.fstride = fstride, a.rstride = rstride, a.win = window, a.lines = nullptr;
            a.nlines = p.nrow, a.out = H;
            if (in_f64) IMCOM_TRY((ns_launch_lines<double, true>(ctx, a)));
            else IMCOM_TRY((ns_launch_lines<float, true>(ctx, a)));
            a.in = nullptr, a.win = nullptr, a.lines = H, a.nlines = p.ncol, a.out = F;
            IMCOM_TRY((ns_launch_lines<double, false>(ctx, a)));
        }
    }
    ProfScope ps(ctx, "noiseps_epilogue");
    const int n = bin8 ? L / 8 : L;
    hipLaunchKernelGGL(ns_epilogue_kernel, dim3((n + 63) / 64, n, nframe), dim3(64), 0, st, (const cplx *)F, L, bin8 ? 1 : 0, norm_dev, out);
    return check_launch("ns_epilogue_kernel");
}

static int launch_noiseps_radial(imcom_ctx *ctx, const double *image, int nframe, int n, const int *rbin, int nidx, double *mean, double *err)
{
    ProfScope ps(ctx, "noiseps_radial");
    hipLaunchKernelGGL(ns_radial_kernel, dim3(nidx, nframe), dim3(256), 0, ctx->stream, image, (long)n * n, rbin, nidx, mean, err);
    return check_launch("ns_radial_kernel");
}

static int launch_noiseps_accumulate(imcom_ctx *ctx, const double *ps2d, const double *mean, const double *err, int nlayers, long npix, int nrad, int bins,
                              int coverage_bin, double *ps2d_all, double *ps1d_all)
{
    const long span = std::max<long>(npix, nrad);
    hipLaunchKernelGGL(ns_accumulate_kernel, dim3((unsigned)((span + 255) / 256), nlayers), dim3(256), 0, ctx->stream, ps2d, mean, err, npix, nrad, bins,
                       coverage_bin, ps2d_all, ps1d_all);
    return check_launch("ns_accumulate_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: noise power spectra of coadded frames

static int noiseps_pick(int L, int route)  // route 0: the plan's own choice (IMCOM_NOISEPS_ROUTE=dense forces the dense DFT)
{
    const int best = noiseps_route(L, env_is("IMCOM_NOISEPS_ROUTE", "dense"));
    if (route == 0 || best == NOISEPS_ROUTE_NONE) return best;
    if (route == NOISEPS_ROUTE_DENSE) return route;
    return route == noiseps_route(L, false) ? route : NOISEPS_ROUTE_NONE;
}

static int noiseps_check_side(int L, int bin8)
{
    IMCOM_REQUIRE(L >= 2 && L % 2 == 0, "noise spectra: the side %d is not even", L);
    IMCOM_REQUIRE(!bin8 || L % 8 == 0, "noise spectra: the side %d is not a multiple of 8 (8 x 8 binning)", L);
    IMCOM_REQUIRE(L <= DFT_DENSE_MAXN, "noise spectra: a side of %d is beyond the %d this build transforms", L, DFT_DENSE_MAXN);
    return IMCOM_OK;
}

extern "C" {

int imcom_noiseps_route(int L) { return noiseps_route(L, env_is("IMCOM_NOISEPS_ROUTE", "dense")); }

int imcom_noiseps_sizes(int L, int nframe, int bin8, int route, long *out)
{
    IMCOM_REQUIRE(out, "null out");
    IMCOM_TRY(noiseps_check_side(L, bin8));
    IMCOM_REQUIRE(nframe >= 1 && nframe <= 65535 && route >= 0 && route <= 3, "noise spectra: %d frames, route %d", nframe, route);
    const int r = noiseps_pick(L, route);
    IMCOM_REQUIRE(r != NOISEPS_ROUTE_NONE, "noise spectra: route %d does not serve the side %d", route, L);
    out[0] = r;
    out[1] = bin8 ? L / 8 : L;
    out[2] = (long)noiseps_ws(L, nframe, r) + (long)nframe * 8 + 4096;
    out[3] = (long)(L / 2 + 1) * L * 16;
    return IMCOM_OK;
}

int imcom_noiseps_2d(imcom_ctx *ctx, const void *frames, int in_f64, int nframe, int L, long fstride, long rstride, const double *window, long window_len,
                     const double *norm, int bin8, int route, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(frames && norm && out, "null pointer");
    IMCOM_TRY(noiseps_check_side(L, bin8));
    IMCOM_REQUIRE(nframe >= 1 && nframe <= 65535 && route >= 0 && route <= 3, "noise spectra: %d frames, route %d", nframe, route);
    IMCOM_REQUIRE(rstride >= L && (nframe == 1 || fstride >= (long)(L - 1) * rstride + L), "noise spectra: strides %ld, %ld of frames of side %d", fstride, rstride, L);
    IMCOM_REQUIRE(!window || window_len == (long)L * L, "noise spectra: a window of %ld elements for frames of side %d", window_len, L);
    for (int f = 0; f < nframe; f++) IMCOM_REQUIRE(std::isfinite(norm[f]) && norm[f] != 0.0, "noise spectra: norm[%d] = %g", f, norm[f]);
    const int r = noiseps_pick(L, route);
    IMCOM_REQUIRE(r != NOISEPS_ROUTE_NONE, "noise spectra: route %d does not serve the side %d", route, L);
    Stage st(ctx, memspace, __func__);
    const size_t esz = in_f64 ? 8 : 4, span = (size_t)(nframe - 1) * fstride + (size_t)(L - 1) * rstride + L, n = bin8 ? L / 8 : L, szO = (size_t)nframe * n * n;
    WsPlan plan;
    plan.add((size_t)nframe * 8);
    st.plan(plan, {span * esz, szO * 8});
    if (st.host && window) plan.add((size_t)L * L * 8);
    plan.add(noiseps_ws(L, nframe, r));
    IMCOM_TRY(ws_reserve(ctx, plan.total + 4096));
    double *norm_d, *o_d;
    const char *f_d;
    const double *w_d;
    IMCOM_TRY(ws_take(ctx, (size_t)nframe, &norm_d, __func__));
    IMCOM_TRY(upload(ctx, norm_d, norm, (size_t)nframe));
    IMCOM_TRY(st.in((const char *)frames, span * esz, &f_d));
    IMCOM_TRY(st.out(out, szO, &o_d));
    IMCOM_TRY(st.in(window, (size_t)L * L, &w_d));
    IMCOM_TRY(launch_noiseps_2d(ctx, f_d, in_f64 != 0, nframe, L, fstride, rstride, w_d, norm_d, bin8 != 0, r, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, szO));
    return st.done();
}

int imcom_noiseps_radial(imcom_ctx *ctx, const double *image, int nframe, int n, const int *rbin, int nidx, double *mean, double *err, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && rbin && mean && err, "null pointer");
    IMCOM_REQUIRE(nframe >= 1 && nframe <= 65535 && n >= 1 && n <= DFT_DENSE_MAXN && nidx >= 1 && nidx <= 65535, "noise spectra: %d frames of side %d, %d annuli", nframe,
                  n, nidx);
    Stage st(ctx, memspace, __func__);
    const size_t npix = (size_t)n * n, szI = (size_t)nframe * npix, szR = (size_t)nframe * nidx;
    WsPlan plan;
    st.plan(plan, {szI * 8, npix * 4, szR * 8, szR * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total + 4096));
    const double *i_d;
    const int *r_d;
    double *m_d, *e_d;
    IMCOM_TRY(st.in(image, szI, &i_d));
    IMCOM_TRY(st.in(rbin, npix, &r_d));
    IMCOM_TRY(st.out(mean, szR, &m_d));
    IMCOM_TRY(st.out(err, szR, &e_d));
    IMCOM_TRY(launch_noiseps_radial(ctx, i_d, nframe, n, r_d, nidx, m_d, e_d));
    IMCOM_TRY(st.back(mean, (const double *)m_d, szR));
    IMCOM_TRY(st.back(err, (const double *)e_d, szR));
    return st.done();
}

int imcom_noiseps_accumulate(imcom_ctx *ctx, const double *ps2d, const double *mean, const double *err, int nlayers, int n, int nrad, int bins, int coverage_bin,
                             double *ps2d_all, double *ps1d_all)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(ps2d && mean && err && ps2d_all && ps1d_all, "null pointer");
    IMCOM_REQUIRE(nlayers >= 1 && nlayers <= 65535 && n >= 1 && n <= DFT_DENSE_MAXN && nrad >= 1 && bins >= 1 && coverage_bin >= 0 && coverage_bin < bins,
                  "noise spectra: %d layers of side %d, %d annuli, coverage bin %d of %d", nlayers, n, nrad, coverage_bin, bins);
    return launch_noiseps_accumulate(ctx, ps2d, mean, err, nlayers, (long)n * n, nrad, bins, coverage_bin, ps2d_all, ps1d_all);
}

}  // extern "C"
