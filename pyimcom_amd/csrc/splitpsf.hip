// splitpsf.hip -- the split of a Legendre PSF cube into a short-range PSF and a long-range kernel on the device.
//
// Replaces the numerical content of SplitPSF (reference src/pyimcom/splitpsf/splitpsf.py): the tophat filter of the constructor
// (tophatfilter, 131-154), the windows and the split (92-128, 223-234) and, per Gauss-Legendre grid point, the Legendre combination (267),
// the Gaussian deconvolution (gauss_deconv, 156-170), the error map zeta (269-274) and the update of K_Legendre (277, 282-284).
//
// Every transform is a cyclic 2-D DFT of complex planes [plane][N][N], done as two passes of ONE primitive: "transform the contiguous
// lines of every plane and store the result transposed" -- after two passes the spectrum is in natural order again.  The primitive has
// two routes: (1) the wave-per-line butterflies of fft_lines.h when N is a side fft_line_plan (fft_plan_core.h) takes: N <= 1024, a
// product of 2, 3, 5; (2) for every other N the dense-DFT line engine of fft.hip (ONE real product on the fp64 MFMA tile engine), then
// a transposing copy.  Both routes compute the same formula.
//
// Determinism: a plane's transforms involve that plane only (a real plane rides as a complex one with a zero imaginary part; in the
// zeta step K_real and its own Gaussian stamp ride together), every output element has one owner thread, and K_Legendre adds its
// grid points in ascending order with separately rounded products and sums: the result is the same bit for bit for every split
// of the grid points and the SCAs into calls.  Only the tophat filter pairs planes (2j, 2j+1 of one cube: a fixed pairing).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "fft_lines.h"
#include "launchers.h"

namespace imcom {

constexpr int SPLITPSF_ROUTE_NONE = 0, SPLITPSF_ROUTE_LINES = 1, SPLITPSF_ROUTE_DENSE = 2;

static int splitpsf_route(int nfft)
{
    if (nfft < 2 || nfft > DFT_DENSE_MAXN) return SPLITPSF_ROUTE_NONE;
    FftPlan pl;
    return fft_line_plan(nfft, &pl) ? SPLITPSF_ROUTE_LINES : SPLITPSF_ROUTE_DENSE;
}

// ---------------------------------------------------------------------------------------------------------
// the primitive, route 1: line L = (plane b, row y) of `in`, transformed, goes to column y of plane b of `out`
template <bool INV>
__global__ __launch_bounds__(WF_MAXWAVES * 64) void sp_lines_kernel(const cplx *__restrict__ in, cplx *__restrict__ out, long nlines, FftPlan pl,
                                                                    const cplx *__restrict__ tw)
{
    const WfWave w = wf_prologue(pl, tw, pl.waves);
    const int n = pl.n;
    const long L = (long)blockIdx.x * pl.waves + w.wave;
    if (L >= nlines) return;  // (no workgroup barrier below)
    const long b = L / n;
    const int y = (int)(L - b * n);
    const cplx *src = in + L * n;
    cplx *dst = out + b * n * n + y;
    auto load0 = [&](int x) { return src[x]; };
    auto storeN = [&](int k, cplx v) { dst[(long)k * n] = v; };
    wf_line<INV>(w.line, w.twl, pl, load0, storeN);
}

// route 2: the dense-DFT line engine (fft.hip) leaves the transformed line (b, y) in row b N + y of C [Mp][Np] -> out[b][k][y]
__global__ void sp_dense_transpose_kernel(const double *__restrict__ C, int N, int Np, cplx *__restrict__ out)
{
    __shared__ cplx tile[16][17];
    const long b = blockIdx.z;
    const int k0 = blockIdx.x * 16, y0 = blockIdx.y * 16, tx = threadIdx.x, ty = threadIdx.y;
    if (y0 + ty < N && k0 + tx < N) {
        const double *p = C + (b * N + y0 + ty) * Np + 2 * (k0 + tx);
        tile[ty][tx] = make_double2(p[0], p[1]);
    }
    __syncthreads();
    if (k0 + ty < N && y0 + tx < N) out[(b * N + k0 + ty) * N + y0 + tx] = tile[tx][ty];
}

// what one 2-D transform engine needs out of the workspace, and the engine itself
struct SpFft {
    int N = 0, route = 0;
    DftDense d;
    FftPlan pl;
    cplx *tw = nullptr;
};

static void sp_fft_plan(SpFft &f, int N, long planes, WsPlan &plan)
{
    f.N = N;
    f.route = splitpsf_route(N);
    if (f.route == SPLITPSF_ROUTE_LINES) {
        fft_line_plan(N, &f.pl);
        plan.add((size_t)N * 16);
    } else {
        dft_dense_plan(f.d, N, planes * N, true, plan);
    }
}

static int sp_fft_take(imcom_ctx *ctx, SpFft &f, const char *who)
{
    if (f.route == SPLITPSF_ROUTE_LINES) {
        IMCOM_TRY(ws_take(ctx, (size_t)f.N, &f.tw, who));
        IMCOM_TRY(fft_line_twiddles(ctx, f.pl, f.tw));
        IMCOM_TRY(fft_line_lds_opt_in((const void *)sp_lines_kernel<false>, fft_line_lds_bytes(f.pl)));
        return fft_line_lds_opt_in((const void *)sp_lines_kernel<true>, fft_line_lds_bytes(f.pl));
    }
    return dft_dense_take(ctx, f.d, true, who);
}

// one pass: the lines of `planes` planes of `in`, transformed, into `out` transposed
static int sp_lines_T(imcom_ctx *ctx, const SpFft &f, const cplx *in, cplx *out, long planes, bool inv)
{
    const int N = f.N;
    const long nlines = planes * N;
    if (f.route == SPLITPSF_ROUTE_LINES) {
        const int W = f.pl.waves;
        const size_t lds = fft_line_lds_bytes(f.pl);
        const unsigned grid = (unsigned)((nlines + W - 1) / W);
        if (inv) hipLaunchKernelGGL(sp_lines_kernel<true>, dim3(grid), dim3(64 * W), lds, ctx->stream, in, out, nlines, f.pl, (const cplx *)f.tw);
        else hipLaunchKernelGGL(sp_lines_kernel<false>, dim3(grid), dim3(64 * W), lds, ctx->stream, in, out, nlines, f.pl, (const cplx *)f.tw);
        return check_launch("sp_lines_kernel");
    }
    IMCOM_TRY(dft_dense_product(ctx, f.d, in, nlines, inv));
    hipLaunchKernelGGL(sp_dense_transpose_kernel, dim3((N + 15) / 16, (N + 15) / 16, (unsigned)planes), dim3(16, 16), 0, ctx->stream, (const double *)f.d.C, N, f.d.Np,
                       out);
    return check_launch("sp_dense_transpose_kernel");
}

// the cyclic 2-D transform of `planes` planes: a -> a (b is scratch), natural order in and out, unnormalised
static int sp_fft2(imcom_ctx *ctx, const SpFft &f, cplx *a, cplx *b, long planes, bool inv)
{
    IMCOM_TRY(sp_lines_T(ctx, f, a, b, planes, inv));
    return sp_lines_T(ctx, f, b, a, planes, inv);
}

// ---------------------------------------------------------------------------------------------------------
// the tophat filter (splitpsf.py:131-154); planes 2j, 2j+1 of the cube ride as one complex plane (the filter is real and even)
__global__ void sp_tophat_pack_kernel(const double *__restrict__ cube, int nplane, int n, int npad, int N, cplx *__restrict__ Z)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, j = blockIdx.z;
    if (x >= N) return;
    const int yy = y - npad, xx = x - npad;
    cplx v = make_double2(0.0, 0.0);
    if (yy >= 0 && yy < n && xx >= 0 && xx < n) {
        const long o = (long)yy * n + xx, pl = (long)n * n;
        v.x = cube[2L * j * pl + o];
        if (2 * j + 1 < nplane) v.y = cube[(2L * j + 1) * pl + o];
    }
    Z[((long)j * N + y) * N + x] = v;
}

__device__ __forceinline__ double sp_sinc(double x) { return x == 0.0 ? 1.0 : sinpi(x) / (M_PI * x); }
__device__ __forceinline__ double sp_freq(int k, int N)  // numpy: u = k / N, u - 1 where u > 0.5
{
    const double u = (double)k / (double)N;
    return u > 0.5 ? u - 1.0 : u;
}

__global__ void sp_tophat_filter_kernel(cplx *__restrict__ Z, int N, double width)
{
    const int kx = blockIdx.x * blockDim.x + threadIdx.x, ky = blockIdx.y, j = blockIdx.z;
    if (kx >= N) return;
    const double s = sp_sinc(sp_freq(kx, N) * width) * sp_sinc(sp_freq(ky, N) * width);
    cplx *p = Z + ((long)j * N + ky) * N + kx;
    *p = make_double2(p->x * s, p->y * s);
}

__global__ void sp_tophat_crop_kernel(const cplx *__restrict__ Z, int nplane, int n, int npad, int N, double *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= n) return;
    const cplx v = Z[((long)(p >> 1) * N + y + npad) * N + x + npad];
    out[((long)p * n + y) * n + x] = ((p & 1) ? v.y : v.x) / ((double)N * (double)N);
}

static int splitpsf_tophat_npad(double width)  // splitpsf.py:134-135
{
    const int npad = (int)std::ceil(width);
    return npad + (4 - npad % 4) % 4;
}

static size_t tophat_ws(int nplane, int n, double width, SpFft *f_out)
{
    const int N = n + 2 * splitpsf_tophat_npad(width), npair = (nplane + 1) / 2;
    SpFft f;
    WsPlan plan;
    sp_fft_plan(f, N, npair, plan);
    plan.add((size_t)npair * N * N * 16);
    plan.add((size_t)npair * N * N * 16);
    if (f_out) *f_out = f;
    return plan.total;
}
static size_t splitpsf_tophat_ws(int nplane, int n, double width) { return tophat_ws(nplane, n, width, nullptr); }

// cube, out [nplane][n][n] in device memory (out may be cube); the caller has reserved splitpsf_tophat_ws() for this
static int launch_splitpsf_tophat(imcom_ctx *ctx, const double *cube, int nplane, int n, double width, double *out)
{
    const int npad = splitpsf_tophat_npad(width), N = n + 2 * npad, npair = (nplane + 1) / 2;
    SpFft f;
    tophat_ws(nplane, n, width, &f);
    IMCOM_TRY(sp_fft_take(ctx, f, __func__));
    cplx *Z, *T;
    IMCOM_TRY(ws_take(ctx, (size_t)npair * N * N, &Z, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)npair * N * N, &T, __func__));
    ProfScope ps(ctx, "splitpsf_tophat");
    const dim3 gN((N + 255) / 256, N, npair);
    hipLaunchKernelGGL(sp_tophat_pack_kernel, gN, dim3(256), 0, ctx->stream, cube, nplane, n, npad, N, Z);
    IMCOM_TRY(check_launch("sp_tophat_pack_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, Z, T, npair, false));
    hipLaunchKernelGGL(sp_tophat_filter_kernel, gN, dim3(256), 0, ctx->stream, Z, N, width);
    IMCOM_TRY(check_launch("sp_tophat_filter_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, Z, T, npair, true));
    hipLaunchKernelGGL(sp_tophat_crop_kernel, dim3((n + 255) / 256, n, nplane), dim3(256), 0, ctx->stream, (const cplx *)Z, nplane, n, npad, N, out);
    return check_launch("sp_tophat_crop_kernel");
}

// ---------------------------------------------------------------------------------------------------------
// the windows and the split (splitpsf.py:71-128, 223-234)
__device__ __forceinline__ double sp_blackman(double x)
{
    const double alpha = 0.08;
    if (x >= 1.0) return 1.0;
    if (x <= -1.0) return 0.0;
    return 0.5 * (x + 1.0) + (0.5 * sinpi(x) + alpha / 4 * sinpi(2.0 * x)) / ((1.0 - alpha) * M_PI);
}

// trunc [n]: the 1-D factor of Truncate_2D_integratedBlackman (host); smallpsf [npoly][ns][ns], resid [npoly][n][n]
__global__ void sp_split_kernel(const double *__restrict__ cube, int npoly, int n, int ns, double r1, double r2, const double *__restrict__ trunc,
                                double *__restrict__ smallpsf, double *__restrict__ resid)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= n) return;
    const double xx = (1 - n) / 2.0 + x, yy = (1 - n) / 2.0 + y, r = sqrt(xx * xx + yy * yy);
    const double W = sp_blackman(-1.0 + 2.0 / (r2 - r1) * (r2 - r)), T = trunc[y] * trunc[x];
    const int ntrim = (n - ns) / 2, ys = y - ntrim, xs = x - ntrim;
    const bool in_small = ys >= 0 && ys < ns && xs >= 0 && xs < ns;
    for (int a = 0; a < npoly; a++) {
        const double c = cube[((long)a * n + y) * n + x];
        if (in_small) smallpsf[((long)a * ns + ys) * ns + xs] = W * c;
        resid[((long)a * n + y) * n + x] = c * (1.0 - W) * T;
    }
}

static int launch_splitpsf_split(imcom_ctx *ctx, const double *cube, int npoly, int n, int ns, double r1, double r2, const double *trunc_dev, double *smallpsf,
                          double *resid)
{
    hipLaunchKernelGGL(sp_split_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, cube, npoly, n, ns, r1, r2, trunc_dev, smallpsf, resid);
    return check_launch("sp_split_kernel");
}

// ---------------------------------------------------------------------------------------------------------
// per grid point.  Plane p = sl * npts + il: SCA sl of the call, grid point i0 + il.
// locLRP (splitpsf.py:267) in ascending plane order
__global__ void sp_loc_kernel(const double *__restrict__ resid, int npoly, long npix, int npts, int i0, const double *__restrict__ lpw,
                              double *__restrict__ loc)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    if (e >= npix) return;
    const int sl = p / npts, i = i0 + p % npts;
    const double *r = resid + (long)sl * npoly * npix + e, *w = lpw + (long)i * npoly;
    double acc = 0.0;
    for (int a = 0; a < npoly; a++) acc += w[a] * r[a * npix];
    loc[(long)p * npix + e] = acc;
}

// gauss_deconv, 161-163: the plane zero padded to 2n x 2n, as a complex plane
__global__ void sp_pad_real_kernel(const double *__restrict__ src, int n, int N, cplx *__restrict__ Z)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= N) return;
    Z[((long)p * N + y) * N + x] = make_double2((y < n && x < n) ? src[((long)p * n + y) * n + x] : 0.0, 0.0);
}

// gauss_deconv, 164-168: u = k / 2n, minus one from k = n on; u along the last axis
__global__ void sp_deconv_filter_kernel(cplx *__restrict__ Z, int n, int npoly, int npts, int i0, const double *__restrict__ cov, double eps)
{
    const int N = 2 * n, kx = blockIdx.x * blockDim.x + threadIdx.x, ky = blockIdx.y, p = blockIdx.z;
    if (kx >= N) return;
    const double *C = cov + ((long)(p / npts) * npoly + i0 + p % npts) * 4;
    double u = (double)kx / (double)N, v = (double)ky / (double)N;
    if (kx >= n) u -= 1.0;
    if (ky >= n) v -= 1.0;
    const double G = exp(-2.0 * (M_PI * M_PI) * (C[0] * (u * u) + C[3] * (v * v) + 2.0 * C[1] * u * v));
    const double h = G / (G * G + eps * eps);
    cplx *q = Z + ((long)p * N + ky) * N + kx;
    *q = make_double2(q->x * h, q->y * h);
}

// gauss_deconv, 169-170: the real part of the inverse, [:n, :n]
__global__ void sp_kreal_kernel(const cplx *__restrict__ Z, int n, double *__restrict__ kreal)
{
    const int N = 2 * n, x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= n) return;
    kreal[((long)p * n + y) * n + x] = Z[((long)p * N + y) * N + x].x / ((double)N * (double)N);
}

// the operands of the linear convolution of 269-274 as ONE complex plane: K_real + i gauss_stamp (172-185), both zero padded to 2n
__global__ void sp_zeta_pack_kernel(const double *__restrict__ kreal, int n, int npoly, int npts, int i0, const double *__restrict__ cov,
                                    cplx *__restrict__ Z)
{
    const int N = 2 * n, x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= N) return;
    cplx v = make_double2(0.0, 0.0);
    if (x < n && y < n) {
        const double *C = cov + ((long)(p / npts) * npoly + i0 + p % npts) * 4;
        const double det = C[0] * C[3] - C[1] * C[1], i00 = C[3] / det, i01 = -C[1] / det, i11 = C[0] / det;
        const double xx = (1 - n) / 2.0 + x, yy = (1 - n) / 2.0 + y;
        v.x = kreal[((long)p * n + y) * n + x];
        v.y = exp(-0.5 * (i00 * (xx * xx) + i11 * (yy * yy)) - i01 * xx * yy) / (2.0 * M_PI * sqrt(det));
    }
    Z[((long)p * N + y) * N + x] = v;
}

// Z = FFT(a + i b), a and b real: A_k = (Z_k + conj Z_-k) / 2, B_k = (Z_k - conj Z_-k) / (2 i); out = A_k B_k
__global__ void sp_zeta_product_kernel(const cplx *__restrict__ Z, int N, cplx *__restrict__ out)
{
    const int kx = blockIdx.x * blockDim.x + threadIdx.x, ky = blockIdx.y, p = blockIdx.z;
    if (kx >= N) return;
    const cplx *pl = Z + (long)p * N * N;
    const cplx z = pl[(long)ky * N + kx], m = pl[(long)((N - ky) % N) * N + (N - kx) % N];
    const cplx A = make_double2(0.5 * (z.x + m.x), 0.5 * (z.y - m.y)), B = make_double2(0.5 * (z.y + m.y), -0.5 * (z.x - m.x));
    out[((long)p * N + ky) * N + kx] = cmulf(A, B);
}

// zeta = locLRP - the "same" part of the convolution (offset (n - 1) / 2); the row's max |zeta| goes to part[p n + y]
__global__ __launch_bounds__(256) void sp_zeta_kernel(const cplx *__restrict__ Z, const double *__restrict__ loc, int n, double *__restrict__ zeta,
                                                      double *__restrict__ part)
{
    __shared__ double red[256];
    const int N = 2 * n, y = blockIdx.x, p = blockIdx.y, off = (n - 1) / 2;
    double mx = 0.0;
    for (int x = threadIdx.x; x < n; x += 256) {
        const long o = ((long)p * n + y) * n + x;
        const double z = loc[o] - Z[((long)p * N + y + off) * N + x + off].x / ((double)N * (double)N);
        if (zeta) zeta[o] = z;
        mx = fmax(mx, fabs(z));
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)p * n + y] = red[0];
}

// zmax[sl] = max(zmax[sl] unless this is the SCA's first grid point, the SCA's row maxima)
__global__ __launch_bounds__(256) void sp_zmax_kernel(const double *__restrict__ part, long per_sca, int first, double *__restrict__ zmax)
{
    __shared__ double red[256];
    const int sl = blockIdx.x;
    double mx = first ? 0.0 : zmax[sl];
    for (long e = threadIdx.x; e < per_sca; e += 256) mx = fmax(mx, part[(long)sl * per_sca + e]);
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) zmax[sl] = red[0];
}

// 277, 282-284: K_Legendre[a] += wg[i] * (lpw_i[a] * K_real_i), i ascending, every product and sum rounded on its own (as numpy does);
// after the last grid point the (l_x + 1/2)(l_y + 1/2) normalisation.  One owner thread per element.
__global__ void sp_accumulate_kernel(const double *__restrict__ kreal, int npoly, long npix, int npts, int i0, const double *__restrict__ lpw,
                                     const double *__restrict__ wg, int lorder1, double *__restrict__ KL)
{
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int a = blockIdx.y, sl = blockIdx.z;
    if (e >= npix) return;
    double *dst = KL + ((long)sl * npoly + a) * npix + e;
    double acc = i0 == 0 ? 0.0 : *dst;
    for (int il = 0; il < npts; il++) {
        const int i = i0 + il;
        const double t = __dmul_rn(lpw[(long)i * npoly + a], kreal[((long)sl * npts + il) * npix + e]);
        acc = __dadd_rn(acc, __dmul_rn(wg[i], t));
    }
    if (i0 + npts == npoly) acc = __dmul_rn(acc, __dmul_rn((a / lorder1) + 0.5, (a % lorder1) + 0.5));
    *dst = acc;
}

static size_t points_ws(int n, int nsca, int npts, bool own_kreal, SpFft *f_out)
{
    const long P = (long)nsca * npts;
    const int N = 2 * n;
    SpFft f;
    WsPlan plan;
    sp_fft_plan(f, N, P, plan);
    plan.add((size_t)P * N * N * 16);          // Z
    plan.add((size_t)P * N * N * 16);          // T
    plan.add((size_t)P * n * n * 8);           // locLRP
    if (own_kreal) plan.add((size_t)P * n * n * 8);
    plan.add((size_t)P * n * 8);               // row maxima of |zeta|
    if (f_out) *f_out = f;
    return plan.total;
}
static size_t splitpsf_points_ws(int n, int nsca, int npts, bool own_kreal) { return points_ws(n, nsca, npts, own_kreal, nullptr); }

// resid [nsca][npoly][n][n]; lpw [npoly][npoly], wg [npoly], cov [nsca][npoly][4] in device memory; K_real / zeta (may be null)
// [nsca][npts][n][n]; KL [nsca][npoly][n][n]; zmax [nsca].  The caller has reserved splitpsf_points_ws() for this.
static int launch_splitpsf_points(imcom_ctx *ctx, const double *resid, int nsca, int npoly, int n, int i0, int npts, const double *lpw, const double *wg,
                           const double *cov, double eps, double *KL, double *K_real, double *zeta, double *zmax)
{
    const long P = (long)nsca * npts, npix = (long)n * n;
    const int N = 2 * n;
    int lorder1 = 1;
    while (lorder1 * lorder1 < npoly) lorder1++;
    SpFft f;
    points_ws(n, nsca, npts, !K_real, &f);
    IMCOM_TRY(sp_fft_take(ctx, f, __func__));
    cplx *Z, *T;
    double *loc, *kreal = K_real, *part;
    IMCOM_TRY(ws_take(ctx, (size_t)P * N * N, &Z, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)P * N * N, &T, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)P * npix, &loc, __func__));
    if (!kreal) IMCOM_TRY(ws_take(ctx, (size_t)P * npix, &kreal, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)P * n, &part, __func__));
    ProfScope ps(ctx, "splitpsf_points");
    hipStream_t st = ctx->stream;
    const dim3 gN((N + 255) / 256, N, (unsigned)P), gn((n + 255) / 256, n, (unsigned)P);
    hipLaunchKernelGGL(sp_loc_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)P), dim3(256), 0, st, resid, npoly, npix, npts, i0, lpw, loc);
    hipLaunchKernelGGL(sp_pad_real_kernel, gN, dim3(256), 0, st, (const double *)loc, n, N, Z);
    IMCOM_TRY(check_launch("sp_pad_real_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, Z, T, P, false));
    hipLaunchKernelGGL(sp_deconv_filter_kernel, gN, dim3(256), 0, st, Z, n, npoly, npts, i0, cov, eps);
    IMCOM_TRY(check_launch("sp_deconv_filter_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, Z, T, P, true));
    hipLaunchKernelGGL(sp_kreal_kernel, gn, dim3(256), 0, st, (const cplx *)Z, n, kreal);
    hipLaunchKernelGGL(sp_zeta_pack_kernel, gN, dim3(256), 0, st, (const double *)kreal, n, npoly, npts, i0, cov, Z);
    IMCOM_TRY(check_launch("sp_zeta_pack_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, Z, T, P, false));
    hipLaunchKernelGGL(sp_zeta_product_kernel, gN, dim3(256), 0, st, (const cplx *)Z, N, T);
    IMCOM_TRY(check_launch("sp_zeta_product_kernel"));
    IMCOM_TRY(sp_fft2(ctx, f, T, Z, P, true));
    hipLaunchKernelGGL(sp_zeta_kernel, dim3(n, (unsigned)P), dim3(256), 0, st, (const cplx *)T, (const double *)loc, n, zeta, part);
    hipLaunchKernelGGL(sp_zmax_kernel, dim3(nsca), dim3(256), 0, st, (const double *)part, (long)npts * n, i0 == 0 ? 1 : 0, zmax);
    hipLaunchKernelGGL(sp_accumulate_kernel, dim3((unsigned)((npix + 255) / 256), npoly, nsca), dim3(256), 0, st, (const double *)kreal, npoly, npix, npts, i0,
                       lpw, wg, lorder1, KL);
    return check_launch("sp_accumulate_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: the split of a PSF cube into its short- and long-range parts

static int splitpsf_lorder1(int npoly)
{
    int l1 = 1;
    while (l1 * l1 < npoly) l1++;
    return l1 * l1 == npoly ? l1 : 0;
}

extern "C" {

int imcom_splitpsf_sizes(int n, int npoly, double width, int nsca, int npts, long *out)
{
    IMCOM_REQUIRE(out, "null out");
    IMCOM_REQUIRE(n >= 1 && n <= 65536 && npoly >= 1 && npoly <= 4096 && nsca >= 1 && npts >= 1 && npts <= npoly && width > 0.0 && width <= 4096.0,
                  "splitpsf: side %d, %d planes, tophat width %g, %d SCAs or %d grid points out of range", n, npoly, width, nsca, npts);
    const int npad = splitpsf_tophat_npad(width);
    out[0] = npad;
    out[1] = n + 2 * npad;
    out[2] = splitpsf_route(n + 2 * npad);
    out[3] = splitpsf_route(2 * n);
    out[4] = out[2] ? (long)splitpsf_tophat_ws(npoly, n, width) + 4096 : 0;
    out[5] = out[3] ? (long)splitpsf_points_ws(n, nsca, npts, true) + (long)(npoly * npoly + npoly + 4L * nsca * npoly) * 8 + 4096 : 0;
    return IMCOM_OK;
}

int imcom_splitpsf_tophat(imcom_ctx *ctx, const double *cube, int nplane, int n, double width, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(cube && out, "null pointer");
    IMCOM_REQUIRE(nplane >= 1 && nplane <= 65535 && n >= 1 && n <= DFT_DENSE_MAXN && width > 0.0 && width <= 4096.0, "splitpsf tophat: %d planes of side %d, width %g",
                  nplane, n, width);
    if (!splitpsf_route(n + 2 * splitpsf_tophat_npad(width))) {
        set_error("splitpsf tophat: a padded side of %d is beyond the %d this build transforms", n + 2 * splitpsf_tophat_npad(width), DFT_DENSE_MAXN);
        return IMCOM_ERR_UNSUPPORTED;
    }
    Stage st(ctx, memspace, __func__);
    const size_t sz = (size_t)nplane * n * n;
    WsPlan plan;
    st.plan(plan, {sz * 8});
    plan.add(splitpsf_tophat_ws(nplane, n, width));
    IMCOM_TRY(ws_reserve(ctx, plan.total + 4096));
    const double *c_d;
    IMCOM_TRY(st.in(cube, sz, &c_d));
    double *o_d = st.host ? (double *)c_d : out;  // the staged copy is filtered in place
    IMCOM_TRY(launch_splitpsf_tophat(ctx, c_d, nplane, n, width, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, sz));
    return st.done();
}

int imcom_splitpsf_split(imcom_ctx *ctx, const double *cube, int npoly, int n, int ns, double r_in, double r_out, int m_trunc, double *smallpsf,
                         double *resid, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(cube && smallpsf && resid, "null pointer");
    IMCOM_REQUIRE(npoly >= 1 && n >= 2 && n <= DFT_DENSE_MAXN && n % 2 == 0 && ns >= 2 && ns <= n && ns % 2 == 0, "SplitPSF requires even dimension (%d, %d)", n, ns);
    IMCOM_REQUIRE(std::isfinite(r_in) && std::isfinite(r_out) && r_in != r_out && m_trunc >= 0 && 2 * m_trunc <= n, "splitpsf: radii %g, %g, m_trunc %d", r_in,
                  r_out, m_trunc);
    // the 1-D factor of Truncate_2D_integratedBlackman (splitpsf.py:122-128), Window_integratedBlackman (79-89) on the host
    std::vector<double> tr((size_t)n, 1.0);
    for (int k = 0; k < m_trunc; k++) {
        const double step = 2.0 / (m_trunc + 1), x = (k + 1) * step + -1.0, alpha = 0.08;
        tr[k] = x >= 1 ? 1.0 : x <= -1 ? 0.0 : 0.5 * (x + 1) + (0.5 * std::sin(M_PI * x) + alpha / 4 * std::sin(2 * M_PI * x)) / ((1 - alpha) * M_PI);
    }
    for (int k = 0; k < m_trunc; k++) tr[n - m_trunc + k] = tr[m_trunc - 1 - k];
    Stage st(ctx, memspace, __func__);
    const size_t szC = (size_t)npoly * n * n, szS = (size_t)npoly * ns * ns;
    WsPlan plan;
    plan.add((size_t)n * 8);
    st.plan(plan, {szC * 8, szS * 8, szC * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total + 4096));
    double *tr_d, *s_d, *r_d;
    const double *c_d;
    IMCOM_TRY(ws_take(ctx, (size_t)n, &tr_d, __func__));
    IMCOM_TRY(upload(ctx, tr_d, tr.data(), (size_t)n));
    IMCOM_TRY(st.in(cube, szC, &c_d));
    IMCOM_TRY(st.out(smallpsf, szS, &s_d));
    IMCOM_TRY(st.out(resid, szC, &r_d));
    IMCOM_TRY(launch_splitpsf_split(ctx, c_d, npoly, n, ns, r_in, r_out, tr_d, s_d, r_d));
    IMCOM_TRY(st.back(smallpsf, (const double *)s_d, szS));
    IMCOM_TRY(st.back(resid, (const double *)r_d, szC));
    return st.done();
}

int imcom_splitpsf_points(imcom_ctx *ctx, const double *resid, int nsca, int npoly, int n, int i0, int npts, const double *lpw, const double *wg,
                          const double *cov, double eps, double *K_Legendre, double *K_real, double *zeta_real, double *zetamax, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(resid && lpw && wg && cov && K_Legendre && zetamax, "null pointer");
    IMCOM_REQUIRE(npoly >= 1 && npoly <= 4096 && splitpsf_lorder1(npoly), "SplitPSF Legendre polynomial dimension error (%d planes)", npoly);
    IMCOM_REQUIRE(n >= 2 && n % 2 == 0, "SplitPSF requires even dimension (%d)", n);
    IMCOM_REQUIRE(nsca >= 1 && i0 >= 0 && npts >= 1 && i0 + npts <= npoly && (long)nsca * npts <= 65535, "splitpsf: %d SCAs, grid points %d .. %d of %d", nsca, i0,
                  i0 + npts, npoly);
    IMCOM_REQUIRE(std::isfinite(eps) && eps >= 0.0, "splitpsf: eps = %g", eps);
    for (long e = 0; e < (long)nsca * npoly; e++) {
        const double *C = cov + 4 * e;
        IMCOM_REQUIRE(C[0] > 0.0 && C[0] * C[3] - C[1] * C[1] > 0.0 && std::isfinite(C[0] + C[1] + C[3]),  // (C[1][0] is not read: 167, 181-182)
                      "splitpsf: covariance %ld is not positive definite", e);
    }
    if (!splitpsf_route(2 * n)) {
        set_error("splitpsf: a cube side of %d needs transforms of %d, beyond the %d this build transforms", n, 2 * n, DFT_DENSE_MAXN);
        return IMCOM_ERR_UNSUPPORTED;
    }
    Stage st(ctx, memspace, __func__);
    const size_t szR = (size_t)nsca * npoly * n * n, szP = (size_t)nsca * npts * n * n, szL = (size_t)npoly * npoly, szC = (size_t)nsca * npoly * 4;
    WsPlan plan;
    plan.add(szL * 8);
    plan.add((size_t)npoly * 8);
    plan.add(szC * 8);
    st.plan(plan, {szR * 8, szR * 8, (size_t)nsca * 8});
    if (st.host && K_real) plan.add(szP * 8);
    if (st.host && zeta_real) plan.add(szP * 8);
    plan.add(splitpsf_points_ws(n, nsca, npts, !K_real));
    IMCOM_TRY(ws_reserve(ctx, plan.total + 4096));
    double *lpw_d, *wg_d, *cov_d, *KL_d, *zm_d, *kr_d = nullptr, *ze_d = nullptr;
    const double *r_d;
    IMCOM_TRY(ws_take(ctx, szL, &lpw_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)npoly, &wg_d, __func__));
    IMCOM_TRY(ws_take(ctx, szC, &cov_d, __func__));
    IMCOM_TRY(upload(ctx, lpw_d, lpw, szL));
    IMCOM_TRY(upload(ctx, wg_d, wg, (size_t)npoly));
    IMCOM_TRY(upload(ctx, cov_d, cov, szC));
    IMCOM_TRY(st.in(resid, szR, &r_d));
    IMCOM_TRY(st.inout(K_Legendre, szR, &KL_d));
    IMCOM_TRY(st.inout(zetamax, (size_t)nsca, &zm_d));
    if (K_real) IMCOM_TRY(st.out(K_real, szP, &kr_d));
    if (zeta_real) IMCOM_TRY(st.out(zeta_real, szP, &ze_d));
    IMCOM_TRY(launch_splitpsf_points(ctx, r_d, nsca, npoly, n, i0, npts, lpw_d, wg_d, cov_d, eps, KL_d, kr_d, ze_d, zm_d));
    IMCOM_TRY(st.back(K_Legendre, (const double *)KL_d, szR));
    IMCOM_TRY(st.back(zetamax, (const double *)zm_d, (size_t)nsca));
    if (K_real) IMCOM_TRY(st.back(K_real, (const double *)kr_d, szP));
    if (zeta_real) IMCOM_TRY(st.back(zeta_real, (const double *)ze_d, szP));
    return st.done();
}

}  // extern "C"
