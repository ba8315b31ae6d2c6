// imsubtract.hip -- the long-range PSF part of an SCA image (reference src/pyimcom/splitpsf/imsubtract.py:658-707, run_imsubtract_single):
// the canvas assembly  canvas[box] += H * area  and the Legendre-modulated convolution of the canvas with the kernel planes, evaluated
// ONLY at the one sample in oversamp^2 that the reference keeps (imsubtract.py:707) and subtracted from the layer in the same launch.
// The C-ABI entries imcom_imsub_* are at the end of the file.
//
// With s = oversamp, np = ax / s and j = s j' + p, i = s i' + q the kept sample (Y, X) is
//   KH[Y][X] = sum_c sum_{p,q < s} sum_{jj,ii < np} Kf[c][p][q][jj][ii] * arr_c[s (Y + Bp + jj) + rho_p][s (X + Bq + ii) + rho_q]
// with Kf[c][p][q][jj][ii] = K[c][s (np-1-jj) + p][s (np-1-ii) + q] (the flipped phase kernel), e_p = first_index + ax - 1 - p,
// rho_p = e_p mod s, Bp = e_p div s - (np - 1): s^2 dense correlations of an (np x np) kernel with a sub-image of unit stride per term c.
#include "launchers.h"

namespace imcom {

constexpr int IMS_TX = 64, IMS_TY = 32;     // output tile of a workgroup: 256 threads, 8 consecutive X each
constexpr int IMS_JC = 64, IMS_IC = 64;     // kernel rows / (padded) columns per pass over the LDS tile
constexpr int IMS_LW = IMS_TX + IMS_IC + 8;  // tile width in floats: TX + IC - 1 columns used, the sliding window reads 8 beyond its last tap
constexpr int IMS_LH = IMS_TY + IMS_JC - 1;

// Kf [Nl^2][s][s][np][npp] (doubles, npp = np rounded up to 8, the padding zero) from K [ncoeff][ax][ax] (float32)
__global__ __launch_bounds__(256) void imsub_prepare_kernel(const float *__restrict__ K, int ax, int s, int np, int npp, long total, double *__restrict__ Kf)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ii = (int)(idx % npp);
    long r = idx / npp;
    const int jj = (int)(r % np);
    r /= np;
    const int q = (int)(r % s);
    r /= s;
    const int p = (int)(r % s);
    const long c = r / s;
    double v = 0.0;
    if (ii < np) v = (double)K[(c * ax + ((long)s * (np - 1 - jj) + p)) * ax + ((long)s * (np - 1 - ii) + q)];
    Kf[idx] = v;
}

struct ImsubGeom {
    int A, s, ax, np, npp, Nl, nside, first;
    int y0, ny;        // output rows of this call
    long crow0, crows;  // canvas rows held: [crow0, crow0 + crows)
};

// One owner per output sample, a fixed order of terms (c, p, q, kernel row, kernel column): no atomics, and the sum of a sample does not
// depend on which call or workgroup evaluates it.  Products and sums are float64 (the float32 canvas and kernel are exact in it).
__global__ __launch_bounds__(256) void imsub_convolve_kernel(const float *__restrict__ canvas, const float *__restrict__ leg, const double *__restrict__ Kf,
                                                             ImsubGeom g, float *__restrict__ image, double *__restrict__ kh)
{
    __shared__ float tile[IMS_LH * IMS_LW];
    const int t = threadIdx.x, tx = t & 7, ty = t >> 3;
    const int X0 = blockIdx.x * IMS_TX, Y0 = g.y0 + blockIdx.y * IMS_TY;
    const int s = g.s, np = g.np, npp = g.npp;
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 0.0;

    for (int c = 0; c < g.Nl * g.Nl; c++) {
        const float *Pu = leg + (long)(c % g.Nl) * g.A, *Pv = leg + (long)(c / g.Nl) * g.A;  // plane lu + lv Nl (imsubtract.py:698)
        for (int p = 0; p < s; p++) {
            const int ep = g.first + g.ax - 1 - p, rp = ep % s, Bp = ep / s - (np - 1);
            for (int q = 0; q < s; q++) {
                const int eq = g.first + g.ax - 1 - q, rq = eq % s, Bq = eq / s - (np - 1);
                const double *Kpq = Kf + (((long)c * s + p) * s + q) * np * npp;
                for (int j0 = 0; j0 < np; j0 += IMS_JC) {
                    const int jc = min(IMS_JC, np - j0);
                    for (int i0 = 0; i0 < npp; i0 += IMS_IC) {
                        const int ic = min(IMS_IC, npp - i0);
                        // gather the phase sub-image, modulated as the reference does it: float32 products, x factor first (imsubtract.py:694-696)
                        const int R0 = Y0 + Bp + j0, C0 = X0 + Bq + i0, cend = X0 + Bq + IMS_TX + np - 1;
                        for (int idx = t; idx < (IMS_TY + jc - 1) * IMS_LW; idx += 256) {
                            const int rr = idx / IMS_LW, cc = idx - rr * IMS_LW;
                            const long r = (long)s * (R0 + rr) + rp, col = (long)s * (C0 + cc) + rq;
                            float v = 0.0f;
                            if (C0 + cc < cend && col < g.A && r >= g.crow0 && r < g.crow0 + g.crows)
                                v = __fmul_rn(__fmul_rn(canvas[(r - g.crow0) * g.A + col], Pu[col]), Pv[r]);
                            tile[idx] = v;
                        }
                        __syncthreads();
                        for (int jj = 0; jj < jc; jj++) {
                            const float *row = tile + (ty + jj) * IMS_LW + tx * 8;
                            const double *kr = Kpq + (long)(j0 + jj) * npp + i0;
                            double w[16];
#pragma unroll
                            for (int k = 0; k < 8; k++) w[k] = (double)row[k];
                            for (int ii0 = 0; ii0 < ic; ii0 += 8) {
#pragma unroll
                                for (int k = 0; k < 8; k++) w[8 + k] = (double)row[ii0 + 8 + k];
#pragma unroll
                                for (int u = 0; u < 8; u++) {
                                    const double kv = kr[ii0 + u];
#pragma unroll
                                    for (int k = 0; k < 8; k++) acc[k] = fma(kv, w[u + k], acc[k]);
                                }
#pragma unroll
                                for (int k = 0; k < 8; k++) w[k] = w[8 + k];
                            }
                        }
                        __syncthreads();
                    }
                }
            }
        }
    }
    const int Y = Y0 + ty;
    if (Y >= g.y0 + g.ny || Y >= g.nside) return;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int X = X0 + tx * 8 + k;
        if (X >= g.nside) continue;
        const long o = (long)(Y - g.y0) * g.nside + X;
        if (kh) kh[o] = acc[k];
        image[o] = (float)((double)image[o] - acc[k]);  // imsubtract.py:707, rounded once
    }
}

// canvas[row0 + j][col0 + i] += H[j][i] * area[j / s][i / s]  (imsubtract.py:665-682: a float64 product added into the float32 canvas)
__global__ __launch_bounds__(256) void imsub_canvas_add_kernel(float *__restrict__ canvas, int A, const double *__restrict__ H, int hh, int hw,
                                                               const float *__restrict__ area, int s, int row0, int col0)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)hh * hw) return;
    const int j = (int)(idx / hw), i = (int)(idx - (long)j * hw);
    float *dst = canvas + (long)(row0 + j) * A + (col0 + i);
    *dst = (float)__dadd_rn((double)*dst, __dmul_rn(H[idx], (double)area[(long)(j / s) * (hw / s) + i / s]));
}

static int launch_imsub_prepare(imcom_ctx *ctx, const float *K, int ax, int s, int Nl, double *Kf)
{
    ProfScope ps(ctx, "imsub_prepare");
    const int np = ax / s, npp = (np + 7) / 8 * 8;
    const long total = (long)Nl * Nl * s * s * np * npp;
    hipLaunchKernelGGL(imsub_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, K, ax, s, np, npp, total, Kf);
    return check_launch("imsub_prepare_kernel");
}

static int launch_imsub_convolve(imcom_ctx *ctx, const float *canvas, int A, long crow0, long crows, const float *leg, const double *Kf, int ax, int Nl, int s,
                          int nside, int first, int y0, int ny, float *image, double *kh)
{
    ProfScope ps(ctx, "imsub_convolve");
    ImsubGeom g;
    g.A = A, g.s = s, g.ax = ax, g.np = ax / s, g.npp = (g.np + 7) / 8 * 8, g.Nl = Nl, g.nside = nside, g.first = first;
    g.y0 = y0, g.ny = ny, g.crow0 = crow0, g.crows = crows;
    hipLaunchKernelGGL(imsub_convolve_kernel, dim3((unsigned)((nside + IMS_TX - 1) / IMS_TX), (unsigned)((ny + IMS_TY - 1) / IMS_TY)), dim3(256), 0,
                       ctx->stream, canvas, leg, Kf, g, image, kh);
    return check_launch("imsub_convolve_kernel");
}

static int launch_imsub_canvas_add(imcom_ctx *ctx, float *canvas, int A, const double *H, int hh, int hw, const float *area, int s, int row0, int col0)
{
    ProfScope ps(ctx, "imsub_canvas_add");
    const long total = (long)hh * hw;
    hipLaunchKernelGGL(imsub_canvas_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, canvas, A, H, hh, hw, area, s, row0, col0);
    return check_launch("imsub_canvas_add_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: the long-range PSF part of an SCA image

extern "C" {

int imcom_imsub_sizes(int ax, int s, int nside, int Nl, long *out)
{
    IMCOM_REQUIRE(out, "null out");
    IMCOM_REQUIRE(s >= 2 && s <= 64 && ax >= s && ax <= 16384 && nside >= 1 && nside <= 65536 && Nl >= 1 && Nl <= 16,
                  "imsubtract: oversamp %d, axis_num %d, nside %d or Nl %d out of range", s, ax, nside, Nl);
    IMCOM_REQUIRE(ax % (2 * s) == 0 || (s % 2 == 1 && ax % s == 0), "axis_num=%d must be a multiple of 2*oversamp, oversamp=%d", ax, s);
    const long ipad = (ax + 2 * s - 1) / (2 * s), np = ax / s, npp = (np + 7) / 8 * 8;  // imsubtract.py:387-389, 451
    out[0] = ipad;
    out[1] = (s + 2 * s * ipad - ax) / 2;
    out[2] = (long)s * (nside + 2 * ipad);
    out[3] = np;
    out[4] = npp;
    out[5] = (long)Nl * Nl * s * s * np * npp;
    return IMCOM_OK;
}

int imcom_imsub_prepare_kernel_f32(imcom_ctx *ctx, const float *K, int ncoeff, int ax, int Nl, int s, double *kf, int memspace)
{
    IMCOM_TRY(enter(ctx));
    long sz[6];
    IMCOM_TRY(imcom_imsub_sizes(ax, s, 1, Nl, sz));
    IMCOM_REQUIRE(K && kf, "null pointer");
    IMCOM_REQUIRE(ncoeff >= 1 && Nl * Nl <= ncoeff, "imsubtract: Nl=%d needs %d kernel planes, the cube has %d", Nl, Nl * Nl, ncoeff);
    Stage st(ctx, memspace, __func__);
    const size_t szK = (size_t)Nl * Nl * ax * ax;
    WsPlan plan;
    st.plan(plan, {szK * 4});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const float *K_d;
    IMCOM_TRY(st.in(K, szK, &K_d));
    IMCOM_TRY(launch_imsub_prepare(ctx, K_d, ax, s, Nl, kf));
    return st.done();
}

int imcom_imsub_canvas_add_f32(imcom_ctx *ctx, float *canvas, int A, const double *H, int hh, int hw, const float *area, int s, int row0, int col0,
                               int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(canvas && H && area, "null pointer");
    IMCOM_REQUIRE(s >= 1 && A >= 1 && A <= 1 << 20 && hh >= 0 && hw >= 0 && hh % s == 0 && hw % s == 0, "imsubtract: the block is %d x %d, oversamp %d", hh,
                  hw, s);
    IMCOM_REQUIRE(row0 >= 0 && col0 >= 0 && (long)row0 + hh <= A && (long)col0 + hw <= A, "imsubtract: block %d x %d at (%d, %d) leaves the %d x %d canvas",
                  hh, hw, row0, col0, A, A);
    if (hh == 0 || hw == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    const size_t szC = (size_t)A * A, szH = (size_t)hh * hw, szA = szH / ((size_t)s * s);
    WsPlan plan;
    st.plan(plan, {szC * 4, szH * 8, szA * 4});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    float *c_d;
    const double *H_d;
    const float *a_d;
    IMCOM_TRY(st.inout(canvas, szC, &c_d));
    IMCOM_TRY(st.in(H, szH, &H_d));
    IMCOM_TRY(st.in(area, szA, &a_d));
    IMCOM_TRY(launch_imsub_canvas_add(ctx, c_d, A, H_d, hh, hw, a_d, s, row0, col0));
    IMCOM_TRY(st.back(canvas, (const float *)c_d, szC));
    return st.done();
}

int imcom_imsub_convolve_subtract_f32(imcom_ctx *ctx, const float *canvas, int A, long crow0, long crows, const float *K, const double *kf, int ncoeff,
                                      int ax, int Nl, int s, int nside, int y0, int ny, float *image, double *kh, int memspace)
{
    IMCOM_TRY(enter(ctx));
    long sz[6];
    IMCOM_TRY(imcom_imsub_sizes(ax, s, nside, Nl, sz));
    const long first = sz[1];
    IMCOM_REQUIRE(canvas && image && (K || kf), "null pointer");
    IMCOM_REQUIRE(ncoeff >= 1 && Nl * Nl <= ncoeff, "imsubtract: Nl=%d needs %d kernel planes, the cube has %d", Nl, Nl * Nl, ncoeff);
    IMCOM_REQUIRE(A == sz[2], "imsubtract: the canvas is %d on a side, oversamp * (nside + 2 * I_pad) = %ld", A, sz[2]);
    IMCOM_REQUIRE(y0 >= 0 && ny >= 0 && (long)y0 + ny <= nside, "imsubtract: rows %d .. %d of an image of %d", y0, y0 + ny, nside);
    if (ny == 0) return IMCOM_OK;
    IMCOM_REQUIRE(crow0 >= 0 && crows >= 1 && crow0 + crows <= A && crow0 <= first + (long)s * y0 && crow0 + crows >= first + (long)s * (y0 + ny - 1) + ax,
                  "imsubtract: canvas rows %ld .. %ld do not cover rows %ld .. %ld", crow0, crow0 + crows, first + (long)s * y0,
                  first + (long)s * (y0 + ny - 1) + ax);
    Stage st(ctx, memspace, __func__);
    const size_t szC = (size_t)crows * A, szK = (size_t)Nl * Nl * ax * ax, szI = (size_t)ny * nside, szL = (size_t)Nl * A;
    WsPlan plan;
    plan.add(szL * 4);
    if (!kf) plan.add((size_t)sz[5] * 8);
    st.plan(plan, {szC * 4, szI * 4});
    if (st.host && !kf) plan.add(szK * 4);
    if (st.host && kh) plan.add(szI * 8);
    IMCOM_TRY(ws_reserve(ctx, plan.total));

    // P_l(u) of the canvas coordinates, float64 rounded to float32 (imsubtract.py:487-488, 695-696)
    std::vector<float> leg(szL);
    {
        const double ipad = (double)sz[0], a = -ipad - 0.5 + 0.5 / s, b = nside + ipad - 0.5 - 0.5 / s, step = (b - a) / (A - 1);
        for (long i = 0; i < A; i++) {
            double x = (double)i * step;  // numpy.linspace: arange * step, then + start; the last sample is the stop itself
            x = x + a;
            if (i == A - 1) x = b;
            const double u = (x - (nside - 1) / 2.0) / (nside / 2.0);
            double pm = 1.0, pc = u;
            for (int l = 0; l < Nl; l++) {
                leg[(size_t)l * A + i] = (float)(l == 0 ? 1.0 : pc);
                if (l >= 1) {
                    const double pn = ((2 * l + 1) * u * pc - l * pm) / (l + 1);
                    pm = pc;
                    pc = pn;
                }
            }
        }
    }
    float *leg_d;
    IMCOM_TRY(ws_take(ctx, szL, &leg_d, __func__));
    IMCOM_TRY(upload(ctx, leg_d, leg.data(), szL));
    double *kf_d = (double *)kf;
    if (!kf) IMCOM_TRY(ws_take(ctx, (size_t)sz[5], &kf_d, __func__));
    const float *c_d;
    float *img_d;
    IMCOM_TRY(st.in(canvas, szC, &c_d));
    IMCOM_TRY(st.inout(image, szI, &img_d));
    if (!kf) {
        const float *K_d;
        IMCOM_TRY(st.in(K, szK, &K_d));
        IMCOM_TRY(launch_imsub_prepare(ctx, K_d, ax, s, Nl, kf_d));
    }
    double *kh_d = nullptr;
    if (kh) IMCOM_TRY(st.out(kh, szI, &kh_d));
    IMCOM_TRY(launch_imsub_convolve(ctx, c_d, A, crow0, crows, leg_d, kf_d, ax, Nl, s, nside, (int)first, y0, ny, img_d, kh_d));
    IMCOM_TRY(st.back(image, (const float *)img_d, szI));
    if (kh) IMCOM_TRY(st.back(kh, (const double *)kh_d, szI));
    return st.done();
}

}  // extern "C"
