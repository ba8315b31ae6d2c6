// ginterp.hip -- the metadetection resampler of pyimcom.meta.ginterp (reference src/pyimcom/meta/ginterp.py) on the device.
//
// InterpMatrix (ginterp.py:19-186) is IMCOM with one system matrix for every output point: the Gaussian overlaps A of the NN grid
// offsets within the search radius, Ad = A + epsilon * (a narrow Gaussian), the corner-0 block Ad[g0, g0] (n_g x n_g) factored ONCE,
// and per output point four Cholesky solves T_c = Ad[g0,g0]^-1 bp[g_c] (one per cell corner, the same matrix for every corner),
// blended bilinearly and normalised.  MultiInterp (ginterp.py:189-340) maps every output pixel to the input grid, builds its T row
// and gathers every layer.
//
// Device layout.  The factor is the library's blocked Cholesky (gemm_f64.hip / chol_diag.hip) on Ad[g0, g0] padded with the
// identity to a multiple of 128, once per call; gi_inv16_kernel then inverts its 16 x 16 diagonal blocks.  cond(Ad) reaches 1e11 at
// Rsearch 6 and an explicit inverse of Ad (or of all of L) loses 5 digits of T, so the per-point solves are true blocked
// substitutions: Y_k = Linv16_k (Bp_k - L[k, :k] Y[:k]), then the same backwards with L^T.  gi_tile_kernel does one tile of
// GI_P = 16 output points per workgroup: the 4 x 16 = 64 right-hand sides are formed in LDS (never in device memory), the two
// sweeps run on them in place (a column per lane, four rows per wave: the L entries a wave needs are uniform, scalar loads), and the
// epilogue blends the corners into T [NN][16] (in the same LDS), forms U and Sigma on the stest points and, for the resampler, the
// mask and the gather of every layer.  T never exists beyond its tile.
//
// The input side of the resampler -- the mosaic of MetaMosaic (reference src/pyimcom/meta/distortimage.py): the paste of the block files,
// the mask cuts and the circles of mask_caps (seam 19) -- follows the resampler's entries and ends the file.
#include <cmath>
#include <vector>

#include "launchers.h"
#include "mosaic_core.h"

namespace imcom {

constexpr int GI_P = 16;               // output points per workgroup
constexpr int GI_COLS = 4 * GI_P;      // right-hand sides per workgroup (corner-major: column = corner * 16 + point)
constexpr int GI_THREADS = 256;
constexpr int GI_MAXG = 256;           // n_g rounded up to 16 (Rsearch 8: n_g = 197 -> 208)
constexpr int GI_MAXNN = 320;          // offsets (Rsearch 8: 232)
constexpr int GI_KPT = GI_MAXNN / 16;  // offsets per thread in the epilogue (16 threads per point)

struct GiParams {
    int NN, ng, ngp, ldl;  // offsets, corner-system size, its multiple of 16, row stride of L
    double a1, c1, m1, s1;  // b  = s1 exp(-(du^2 + dv^2)), du = a1 (posx - x), dv = c1 ((posy + m1 posx) - (y + m1 x))  (ginterp.py:118-127)
    double a2, c2, m2, s2;  // bp = b + s2 exp(...) with the regularisation's coefficients                           (ginterp.py:130-144)
    double inv_ratio;       // 1 / ratio_sqrtdet (ginterp.py:103, 175)
    int stest;
    long blocksize;  // resampler: the chunk of the stest rule (<= 0: the matrix form, rule on the point index itself)
};

struct GiResample {
    int nlayer, ny_in, nx_in, nx, f64, bb;
    double t00, t01, t10, t11, o0, o1;
    const void *in;
    const unsigned char *in_mask;
    void *out;
    unsigned char *out_mask;
    unsigned long long *umax_bits;  // [2]: Umax, Smax as the bits of non-negative doubles (atomicMax orders them)
};

// posx, posy of the offsets as doubles; gidx[c][j] = offset of the j-th member of g_c (-1: padding row); posc[c][k] = j or -1
__global__ __launch_bounds__(GI_THREADS) void gi_tile_kernel(GiParams P, const double *__restrict__ posx, const double *__restrict__ posy,
                                                             const int *__restrict__ gidx, const int *__restrict__ posc,
                                                             const double *__restrict__ L, const double *__restrict__ Linv16,
                                                             const double *__restrict__ A, int npts, const double *__restrict__ xin,
                                                             const double *__restrict__ yin, double *__restrict__ Tout,
                                                             double *__restrict__ Uout, double *__restrict__ Sout, GiResample R)
{
    extern __shared__ double Y[];  // [ngp][64] right-hand sides -> solutions; then T [NN][16]
    __shared__ double xf_s[GI_P], yf_s[GI_P];
    __shared__ int xi_s[GI_P], yi_s[GI_P], edge_s[GI_P];
    const int tid = threadIdx.x, p0 = blockIdx.x * GI_P;
    const bool resample = R.out != nullptr;

    // output positions; the resampler maps them as ginterp.py:279-292 does, left to right and unfused
    if (tid < GI_P) {
        const int i = p0 + tid;
        double xf = 0.0, yf = 0.0;
        int xi = 0, yi = 0, edge = 1;
        if (i < npts) {
            if (resample) {
                const double yo = (double)(i / R.nx), xo = (double)(i % R.nx);
                const double x_in = __dadd_rn(__dadd_rn(__dmul_rn(R.t00, xo), __dmul_rn(R.t01, yo)), R.o0);
                const double y_in = __dadd_rn(__dadd_rn(__dmul_rn(R.t10, xo), __dmul_rn(R.t11, yo)), R.o1);
                // the integer cells as numpy's int32 cast gives them (ginterp.py:289-292), kept in double: a position that is not finite
                // or lies beyond the int32 range gets INT32_MIN, so the edge test masks it and its fraction makes its T (and U) NaN --
                // the reference's Umax / Smax skip such points.  Only cells whose whole search disc lies inside the input are ever
                // converted to int and gathered.
                double fx = floor(x_in), fy = floor(y_in);
                if (!(fx >= -2147483648.0 && fx <= 2147483647.0)) fx = -2147483648.0;
                if (!(fy >= -2147483648.0 && fy <= 2147483647.0)) fy = -2147483648.0;
                edge = (fx >= (double)R.bb && fx + 1.0 + R.bb < (double)R.nx_in && fy >= (double)R.bb && fy + 1.0 + R.bb < (double)R.ny_in) ? 0 : 1;
                xi = edge ? R.bb : (int)fx;  // edge pixels move to bb (ginterp.py:315-316)
                yi = edge ? R.bb : (int)fy;
                xf = x_in - fx;
                yf = y_in - fy;
            } else {
                xf = xin[i];
                yf = yin[i];
            }
        }
        xf_s[tid] = xf;
        yf_s[tid] = yf;
        xi_s[tid] = xi;
        yi_s[tid] = yi;
        edge_s[tid] = edge;
    }
    __syncthreads();

    // right-hand sides bp[g_c] of the 64 columns (padding rows: 0)
    const int ngp = P.ngp;
    for (int idx = tid; idx < ngp * GI_COLS; idx += GI_THREADS) {
        const int j = idx / GI_COLS, c = idx % GI_COLS, corner = c / GI_P, p = c % GI_P;
        const int k = gidx[corner * ngp + j];
        double v = 0.0;
        if (k >= 0) {
            const double px = posx[k], py = posy[k], x = xf_s[p], y = yf_s[p];
            const double du1 = P.a1 * px - P.a1 * x, dv1 = P.c1 * (py + P.m1 * px) - P.c1 * (y + P.m1 * x);
            const double du2 = P.a2 * px - P.a2 * x, dv2 = P.c2 * (py + P.m2 * px) - P.c2 * (y + P.m2 * x);
            v = P.s1 * exp(-(du1 * du1 + dv1 * dv1)) + P.s2 * exp(-(du2 * du2 + dv2 * dv2));
        }
        Y[idx] = v;
    }
    __syncthreads();

    // forward sweep L Y = Bp, then backward L^T X = Y, by blocks of 16 rows: lane = column, wave = 4 rows of the block
    const int col = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), nb = ngp / 16, ldl = P.ldl;
    for (int kb = 0; kb < nb; kb++) {
        const int r0 = kb * 16 + wv * 4;
        double acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = Y[(r0 + q) * GI_COLS + col];
        const double *L0 = L + (long)r0 * ldl;
#pragma unroll 4
        for (int j = 0; j < kb * 16; j++) {
            const double y = Y[j * GI_COLS + col];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] -= L0[(long)q * ldl + j] * y;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) Y[(r0 + q) * GI_COLS + col] = acc[q];
        __syncthreads();
        double z[16];
#pragma unroll
        for (int m = 0; m < 16; m++) z[m] = Y[(kb * 16 + m) * GI_COLS + col];
        const double *D = Linv16 + kb * 256 + wv * 4 * 16;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 16; m++) s += D[q * 16 + m] * z[m];  // (upper part of the inverse block is 0)
            acc[q] = s;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) Y[(r0 + q) * GI_COLS + col] = acc[q];
        __syncthreads();
    }
    for (int kb = nb - 1; kb >= 0; kb--) {
        const int r0 = kb * 16 + wv * 4;
        double acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = Y[(r0 + q) * GI_COLS + col];
#pragma unroll 4
        for (int j = (kb + 1) * 16; j < ngp; j++) {
            const double y = Y[j * GI_COLS + col];
            const double *Lj = L + (long)j * ldl + r0;
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] -= Lj[q] * y;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) Y[(r0 + q) * GI_COLS + col] = acc[q];
        __syncthreads();
        double z[16];
#pragma unroll
        for (int m = 0; m < 16; m++) z[m] = Y[(kb * 16 + m) * GI_COLS + col];
        const double *D = Linv16 + kb * 256 + wv * 4;  // (Linv16_k)^T: row r of the transpose = column r
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 16; m++) s += D[m * 16 + q] * z[m];
            acc[q] = s;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) Y[(r0 + q) * GI_COLS + col] = acc[q];
        __syncthreads();
    }

    // blend the corners (ginterp.py:148-172): TT[k] = sum_c w_c X_c[k], T = TT / sum_k TT[k]; 16 threads per point, k = s mod 16
    const int p = tid >> 4, s = tid & 15, i = p0 + p;
    const double x = xf_s[p], y = yf_s[p];
    const double w[4] = {(1.0 - x) * (1.0 - y), x * (1.0 - y), (1.0 - x) * y, x * y};
    const int NN = P.NN;
    double tv[GI_KPT];
    double part = 0.0;
#pragma unroll
    for (int m = 0; m < GI_KPT; m++) {
        const int k = s + 16 * m;
        double t = 0.0;
        if (k < NN) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int j = posc[c * NN + k];
                if (j >= 0) t += w[c] * Y[j * GI_COLS + c * GI_P + p];
            }
        }
        tv[m] = t;
        part += t;
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) part += __shfl_xor(part, o, 16);
    const double rs = 1.0 / part;
    __syncthreads();
#pragma unroll
    for (int m = 0; m < GI_KPT; m++) {
        const int k = s + 16 * m;
        if (k < NN) {
            tv[m] *= rs;
            Y[k * GI_P + p] = tv[m];
        }
    }
    __syncthreads();
    const double *T = Y;  // [NN][16]

    if (!resample && i < npts) {
        double *to = Tout + (long)i * NN;
#pragma unroll
        for (int m = 0; m < GI_KPT; m++)
            if (s + 16 * m < NN) to[s + 16 * m] = tv[m];
    }

    // U = 1/ratio + sum_k (T A - 2 b^T)_k T_k and Sigma = sum T^2 on the points the reference evaluates (ginterp.py:174-185)
    const long chunk_idx = P.blocksize > 0 ? (long)i % P.blocksize : (long)i;
    if (i < npts && chunk_idx % P.stest == 0) {
        double su = 0.0, ss = 0.0;
#pragma unroll
        for (int m = 0; m < GI_KPT; m++) {
            const int k = s + 16 * m;
            if (k < NN) {
                const double *Ak = A + (long)k * NN;
                double at = 0.0;
                for (int n = 0; n < NN; n++) at += T[n * GI_P + p] * Ak[n];
                const double px = posx[k], py = posy[k];
                const double du1 = P.a1 * px - P.a1 * x, dv1 = P.c1 * (py + P.m1 * px) - P.c1 * (y + P.m1 * x);
                const double b = P.s1 * exp(-(du1 * du1 + dv1 * dv1));
                su += (at - 2.0 * b) * tv[m];
                ss += tv[m] * tv[m];
            }
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
            su += __shfl_xor(su, o, 16);
            ss += __shfl_xor(ss, o, 16);
        }
        const double U = P.inv_ratio + su;
        if (s == 0) {
            if (resample) {
                atomicMax(R.umax_bits, (unsigned long long)__double_as_longlong(fmax(U, 0.0)));
                atomicMax(R.umax_bits + 1, (unsigned long long)__double_as_longlong(fmax(ss, 0.0)));
            } else {
                Uout[i / P.stest] = U;
                Sout[i / P.stest] = ss;
            }
        }
    }
    if (!resample) return;

    // mask (ginterp.py:298-319) and the gather of every layer, k ascending (ginterp.py:318-328)
    const int xi = xi_s[p], yi = yi_s[p];
    int msk = edge_s[p];
    if (i < npts) {
#pragma unroll
        for (int m = 0; m < GI_KPT; m++) {
            const int k = s + 16 * m;
            if (k < NN) {
                const int yy = yi + (int)posy[k], xx = xi + (int)posx[k];  // (only a pixel moved to bb can reach past the edge; it is masked)
                if (yy >= 0 && yy < R.ny_in && xx >= 0 && xx < R.nx_in) msk |= R.in_mask[(long)yy * R.nx_in + xx] ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) msk |= __shfl_xor(msk, o, 16);
    if (i >= npts) return;
    if (s == 0) R.out_mask[i] = (unsigned char)msk;
    const long plane = (long)R.ny_in * R.nx_in, npix = npts;
    for (int l = s; l < R.nlayer; l += 16) {
        if (R.f64) {
            const double *in = (const double *)R.in + l * plane;
            double acc = 0.0;
            if (!msk)
                for (int k = 0; k < NN; k++)
                    acc = __dadd_rn(acc, __dmul_rn(T[k * GI_P + p], in[(long)(yi + (int)posy[k]) * R.nx_in + (xi + (int)posx[k])]));
            ((double *)R.out)[l * npix + i] = acc;
        } else {
            const float *in = (const float *)R.in + l * plane;
            float acc = 0.0f;  // numpy's in-place += of a float64 product into float32: the sum in float64, rounded every term
            if (!msk)
                for (int k = 0; k < NN; k++)
                    acc = (float)__dadd_rn((double)acc,
                                           __dmul_rn(T[k * GI_P + p], (double)in[(long)(yi + (int)posy[k]) * R.nx_in + (xi + (int)posx[k])]));
            ((float *)R.out)[l * npix + i] = acc;
        }
    }
}

// Ad[g0, g0] padded with the identity to ldl, its diagonal, and A [NN][NN] (ginterp.py:85-99)
__global__ void gi_system_kernel(int NN, int ng, int ldl, double sigma, double epsilon, const double *__restrict__ posx,
                                 const double *__restrict__ posy, const int *__restrict__ g0, double *__restrict__ Ad,
                                 double *__restrict__ dg, double *__restrict__ A)
{
    const int r = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
    const double sige2 = 0.5, s2 = sigma * sigma;
    if (c < ldl && r < ldl) {
        double v = (r == c) ? 1.0 : 0.0;
        if (r < ng && c < ng) {
            const int a = g0[r], b = g0[c];
            const double dx = posx[a] - posx[b], dy = posy[a] - posy[b];
            const double ov = (r == c) ? 1.0 : exp(-(dx * dx) / 4.0 / s2) * exp(-(dy * dy) / 4.0 / s2);
            v = ov + epsilon * ((r == c) ? 1.0 : exp(-(dx * dx) / 4.0 / sige2) * exp(-(dy * dy) / 4.0 / sige2));
        }
        Ad[(long)r * ldl + c] = v;
        if (r == c) dg[r] = v;
    }
    if (c < NN && r < NN) {
        const double dx = posx[r] - posx[c], dy = posy[r] - posy[c];
        A[(long)r * NN + c] = (r == c) ? 1.0 : exp(-(dx * dx) / 4.0 / s2) * exp(-(dy * dy) / 4.0 / s2);
    }
}

// inverses of the 16 x 16 diagonal blocks of L (lower): a column per thread, forward substitution
__global__ void gi_inv16_kernel(const double *__restrict__ L, int ldl, double *__restrict__ Linv16)
{
    const int kb = blockIdx.x, c = threadIdx.x;
    if (c >= 16) return;
    const double *Lb = L + (long)kb * 16 * ldl + kb * 16;
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < r; j++) v -= Lb[(long)r * ldl + j] * x[j];
        x[r] = (r < c) ? 0.0 : v / Lb[(long)r * ldl + r];
    }
#pragma unroll
    for (int r = 0; r < 16; r++) Linv16[kb * 256 + r * 16 + c] = x[r];
}

}  // namespace imcom

using namespace imcom;

namespace {

struct GiGeom {
    std::vector<int> posx, posy, g[4];
    double R2;
};

// ginterp.py:62-83 and the corner subsets of :157-159, in the reference's order (row-major meshgrid, filtered)
GiGeom gi_geometry(double Rsearch)
{
    GiGeom G;
    const double R = std::sqrt(std::ceil(Rsearch * Rsearch) + 0.01);
    const int N = (int)(std::ceil(R) + 1) * 2;
    G.R2 = R * R;
    for (int iy = 0; iy < N; iy++)
        for (int ix = 0; ix < N; ix++) {
            const double px = -(N / 2) + 1 + ix, py = -(N / 2) + 1 + iy;
            const double ex = std::fabs(px - 0.5) - 0.5, ey = std::fabs(py - 0.5) - 0.5;
            if (ex * ex + ey * ey <= G.R2) {
                G.posx.push_back((int)px);
                G.posy.push_back((int)py);
            }
        }
    const double xc[4] = {0.0, 1.0, 0.0, 1.0}, yc[4] = {0.0, 0.0, 1.0, 1.0};
    for (int c = 0; c < 4; c++)
        for (size_t k = 0; k < G.posx.size(); k++) {
            const double dx = G.posx[k] - xc[c], dy = G.posy[k] - yc[c];
            if (dx * dx + dy * dy <= G.R2) G.g[c].push_back((int)k);
        }
    return G;
}

// everything one call needs on the device: geometry tables, the factor, its 16 x 16 inverses, A
struct GiSystem {
    GiParams P;
    double *posx, *posy, *L, *Linv16, *A;
    int *gidx, *posc;
};

size_t gi_system_bytes(const GiGeom &G)
{
    const size_t NN = G.posx.size(), ng = G.g[0].size(), ldl = align_up(ng, NB), ngp = align_up(ng, 16);
    return 2 * ldl * ldl * 8 + ldl * 8 + (ldl / NB) * NB * NB * 8 + (ngp / 16) * 256 * 8 + NN * NN * 8 + 2 * NN * 8 + 4 * ngp * 4 + 4 * NN * 4
           + ng * 4 + 64 + 16 * 256;
}

// checked BEFORE the geometry is built: the offset grid grows as Rsearch^2 and a NaN would reach an int conversion
constexpr double GI_MAX_RSEARCH = 64.0;
int gi_check_args(double Rsearch, double samp)
{
    IMCOM_REQUIRE(std::isfinite(Rsearch) && Rsearch > 0.0 && std::isfinite(samp) && samp > 0.0, "ginterp: bad Rsearch %g / samp %g", Rsearch, samp);
    if (Rsearch >= GI_MAX_RSEARCH) {
        set_error("ginterp: Rsearch %g is beyond what this build serves (NN <= %d offsets)", Rsearch, GI_MAXNN);
        return IMCOM_ERR_UNSUPPORTED;
    }
    return IMCOM_OK;
}

int gi_check_range(const GiGeom &G, double Rsearch)
{
    const int NN = (int)G.posx.size(), ng = (int)G.g[0].size();
    if (NN > GI_MAXNN || (int)align_up(ng, 16) > GI_MAXG || NN * GI_P > (int)align_up(ng, 16) * GI_COLS) {
        set_error("ginterp: Rsearch %g gives NN = %d offsets, corner system %d (this build serves NN <= %d, n_g <= %d)", Rsearch, NN, ng,
                  GI_MAXNN, GI_MAXG);
        return IMCOM_ERR_UNSUPPORTED;
    }
    return IMCOM_OK;
}

// workspace must have been reserved (gi_system_bytes) by the caller
int gi_system(imcom_ctx *ctx, const GiGeom &G, double samp, const double *Cov, double epsilon, GiSystem &S)
{
    const int NN = (int)G.posx.size(), ng = (int)G.g[0].size(), ldl = (int)align_up(ng, NB), ngp = (int)align_up(ng, 16);
    const double sigma = samp / std::sqrt(8 * std::log(2.0)), s2 = sigma * sigma;
    const double Cxx = Cov[0], Cxy = Cov[1], Cyy = Cov[2];
    GiParams &P = S.P;
    P.NN = NN; P.ng = ng; P.ngp = ngp; P.ldl = ldl;
    {  // ginterp.py:102-144
        const double detCT = (2 * s2 + Cxx) * (2 * s2 + Cyy) - Cxy * Cxy;
        const double ratio = std::sqrt((s2 + Cxx) * (s2 + Cyy) - Cxy * Cxy) / s2;
        const double ixx = (2 * s2 + Cyy) / detCT, ixy = -Cxy / detCT, iyy = (2 * s2 + Cxx) / detCT;
        P.a1 = std::sqrt((ixx - ixy * ixy / iyy) / 2.0); P.c1 = std::sqrt(iyy / 2.0); P.m1 = ixy / iyy;
        P.s1 = 2 * s2 / std::sqrt(detCT);
        P.inv_ratio = 1.0 / ratio;
        const double se2 = 0.5;
        const double detE = (2 * se2 + Cxx) * (2 * se2 + Cyy) - Cxy * Cxy;
        const double jxx = (2 * se2 + Cyy) / detE, jxy = -Cxy / detE, jyy = (2 * se2 + Cxx) / detE;
        P.a2 = std::sqrt((jxx - jxy * jxy / jyy) / 2.0); P.c2 = std::sqrt(jyy / 2.0); P.m2 = jxy / jyy;
        P.s2 = epsilon * 2 * se2 / std::sqrt(detE);
    }
    const int nbl = ldl / NB;
    double *Ad = (double *)ws_take(ctx, (size_t)ldl * ldl * 8), *dg = (double *)ws_take(ctx, (size_t)ldl * 8);
    S.L = (double *)ws_take(ctx, (size_t)ldl * ldl * 8);
    double *Dinv = (double *)ws_take(ctx, (size_t)nbl * NB * NB * 8);
    S.Linv16 = (double *)ws_take(ctx, (size_t)(ngp / 16) * 256 * 8);
    S.A = (double *)ws_take(ctx, (size_t)NN * NN * 8);
    S.posx = (double *)ws_take(ctx, (size_t)NN * 8);
    S.posy = (double *)ws_take(ctx, (size_t)NN * 8);
    S.gidx = (int *)ws_take(ctx, (size_t)4 * ngp * 4);
    S.posc = (int *)ws_take(ctx, (size_t)4 * NN * 4);
    int *g0 = (int *)ws_take(ctx, (size_t)ng * 4), *ints = (int *)ws_take(ctx, 64);
    if (!Ad || !dg || !S.L || !Dinv || !S.Linv16 || !S.A || !S.posx || !S.posy || !S.gidx || !S.posc || !g0 || !ints) return ws_short("ginterp");
    std::vector<double> px(NN), py(NN);
    std::vector<int> gidx((size_t)4 * ngp, -1), posc((size_t)4 * NN, -1);
    for (int k = 0; k < NN; k++) { px[k] = G.posx[k]; py[k] = G.posy[k]; }
    for (int c = 0; c < 4; c++) {
        if ((int)G.g[c].size() != ng) { set_error("internal: corner subsets differ in size"); return IMCOM_ERR_ARG; }
        for (int j = 0; j < ng; j++) {
            gidx[(size_t)c * ngp + j] = G.g[c][j];
            posc[(size_t)c * NN + G.g[c][j]] = j;
        }
    }
    IMCOM_TRY(upload(ctx, S.posx, px.data(), NN));
    IMCOM_TRY(upload(ctx, S.posy, py.data(), NN));
    IMCOM_TRY(upload(ctx, S.gidx, gidx.data(), gidx.size()));
    IMCOM_TRY(upload(ctx, S.posc, posc.data(), posc.size()));
    IMCOM_TRY(upload(ctx, g0, G.g[0].data(), (size_t)ng));
    const int nblk_h[2] = {nbl, 0};
    int *nblk = ints, *fail = ints + 1;
    IMCOM_TRY(upload(ctx, nblk, nblk_h, 2));  // fail = 0
    const int span = std::max(ldl, NN);
    hipLaunchKernelGGL(gi_system_kernel, dim3((span + 127) / 128, span), dim3(128), 0, ctx->stream, NN, ng, ldl, sigma, epsilon, S.posx, S.posy, g0,
                       Ad, dg, S.A);
    IMCOM_TRY(check_launch("gi_system_kernel"));
    for (int k = 0; k < nbl; k++) {  // the library's blocked Cholesky, one matrix
        IMCOM_TRY(launch_chol_update(ctx, Ad, S.L, ldl, k, nbl, 1, 1, nblk, dg, nullptr, 1));
        IMCOM_TRY(launch_chol_diag(ctx, S.L, Dinv, ldl, k, 1, nblk, fail));
        IMCOM_TRY(launch_chol_trsm(ctx, S.L, Dinv, ldl, k, nbl, 1, nblk));
    }
    hipLaunchKernelGGL(gi_inv16_kernel, dim3(ngp / 16), dim3(64), 0, ctx->stream, S.L, ldl, S.Linv16);
    IMCOM_TRY(check_launch("gi_inv16_kernel"));
    int fail_h = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(&fail_h, fail, 4, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (fail_h) {
        set_error("ginterp: Ad is not positive definite (column %d; scipy's cho_factor raises LinAlgError)", fail_h);
        return IMCOM_ERR_NUMERIC;
    }
    return IMCOM_OK;
}

int gi_launch_tiles(imcom_ctx *ctx, const GiSystem &S, int npts, const double *xin, const double *yin, double *T, double *U, double *Sg,
                    const GiResample &R)
{
    if (npts <= 0) return IMCOM_OK;
    static bool attr_set = false;
    if (!attr_set) {
        IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)gi_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            GI_MAXG * GI_COLS * (int)sizeof(double)));
        attr_set = true;
    }
    const size_t lds = (size_t)S.P.ngp * GI_COLS * sizeof(double);
    ProfScope ps(ctx, "ginterp");
    hipLaunchKernelGGL(gi_tile_kernel, dim3((npts + GI_P - 1) / GI_P), dim3(GI_THREADS), lds, ctx->stream, S.P, S.posx, S.posy, S.gidx, S.posc,
                       S.L, S.Linv16, S.A, npts, xin, yin, T, U, Sg, R);
    return check_launch("gi_tile_kernel");
}

}  // namespace

extern "C" int imcom_ginterp_geometry(double Rsearch, int cap, int *NN, int *ng, int *posx, int *posy, int *corners)
{
    IMCOM_REQUIRE(NN && ng, "ginterp geometry: bad arguments");
    IMCOM_TRY(gi_check_args(Rsearch, 1.0));
    const GiGeom G = gi_geometry(Rsearch);
    *NN = (int)G.posx.size();
    *ng = (int)G.g[0].size();
    if (!posx && !posy && !corners) return IMCOM_OK;
    IMCOM_REQUIRE(cap >= *NN, "ginterp geometry: capacity %d < NN = %d", cap, *NN);
    for (int k = 0; k < *NN; k++) {
        if (posx) posx[k] = G.posx[k];
        if (posy) posy[k] = G.posy[k];
    }
    if (corners)
        for (int c = 0; c < 4; c++)
            for (int j = 0; j < *ng; j++) corners[c * *ng + j] = G.g[c][j];
    return IMCOM_OK;
}

extern "C" int imcom_ginterp_matrix(imcom_ctx *ctx, double Rsearch, double samp, int npts, const double *x_out, const double *y_out,
                                    const double *Cov, double epsilon, int stest, double *T, double *U, double *Sigma, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(npts >= 0 && Cov && stest >= 1 && (npts == 0 || (x_out && y_out && T && U && Sigma)), "ginterp_matrix: bad arguments");
    IMCOM_TRY(gi_check_args(Rsearch, samp));
    const GiGeom G = gi_geometry(Rsearch);
    IMCOM_TRY(gi_check_range(G, Rsearch));
    Stage st(ctx, memspace, __func__);
    const size_t NN = G.posx.size(), nu = ((size_t)npts + stest - 1) / stest;
    const size_t szX = (size_t)npts, szT = (size_t)npts * NN;
    WsPlan plan;
    plan.add(gi_system_bytes(G) + 4096);
    st.plan(plan, {szX * 8, szX * 8, szT * 8, nu * 8, nu * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    GiSystem S;
    IMCOM_TRY(gi_system(ctx, G, samp, Cov, epsilon, S));
    S.P.stest = stest;
    S.P.blocksize = 0;
    const double *xd, *yd;
    double *Td, *Ud, *Sd;
    IMCOM_TRY(st.in(x_out, szX, &xd));
    IMCOM_TRY(st.in(y_out, szX, &yd));
    IMCOM_TRY(st.out(T, szT, &Td));
    IMCOM_TRY(st.out(U, nu, &Ud));
    IMCOM_TRY(st.out(Sigma, nu, &Sd));
    GiResample R{};
    IMCOM_TRY(gi_launch_tiles(ctx, S, npts, xd, yd, Td, Ud, Sd, R));
    IMCOM_TRY(st.back(T, Td, szT));
    IMCOM_TRY(st.back(U, Ud, nu));
    IMCOM_TRY(st.back(Sigma, Sd, nu));
    return st.done();
}

extern "C" int imcom_ginterp_resample(imcom_ctx *ctx, int nlayer, int ny_in, int nx_in, const void *in, int in_f64, const unsigned char *in_mask,
                                      int ny, int nx, const double *origin, const double *transform, double Rsearch, double samp,
                                      const double *Cov, double epsilon, int stest, long blocksize, void *out, unsigned char *out_mask,
                                      double *UmaxSmax, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(nlayer >= 1 && ny_in >= 1 && nx_in >= 1 && in && in_mask && ny >= 0 && nx >= 0 && origin && transform && Cov && stest >= 1 &&
                      blocksize >= 1 && out && out_mask && UmaxSmax && (in_f64 == 0 || in_f64 == 1),
                  "ginterp_resample: bad arguments");
    IMCOM_REQUIRE((long)ny * nx < (1L << 31) && (long)ny_in * nx_in * nlayer < (1L << 40), "ginterp_resample: arrays too large");
    IMCOM_TRY(gi_check_args(Rsearch, samp));
    const GiGeom G = gi_geometry(Rsearch);
    IMCOM_TRY(gi_check_range(G, Rsearch));
    Stage st(ctx, memspace, __func__);
    const int npts = ny * nx, es = in_f64 ? 8 : 4;
    const size_t szIn = (size_t)nlayer * ny_in * nx_in * es, szM = (size_t)ny_in * nx_in, szOut = (size_t)nlayer * npts * es, szOM = (size_t)npts;
    int bb = 0;  // ginterp.py:298-302
    for (size_t k = 0; k < G.posx.size(); k++)
        bb = std::max({bb, -G.posx[k], G.posx[k] - 1, -G.posy[k], G.posy[k] - 1});
    if (2 * bb >= std::min(nx_in, ny_in) || npts == 0) {  // the reference's early exit: all zeros, everything masked
        if (st.host) {
            memset(out, 0, szOut);
            memset(out_mask, 1, szOM);
            UmaxSmax[0] = UmaxSmax[1] = 0.0;
        } else {
            IMCOM_HIP_CHECK(hipMemsetAsync(out, 0, szOut, ctx->stream));
            IMCOM_HIP_CHECK(hipMemsetAsync(out_mask, 1, szOM, ctx->stream));
            IMCOM_HIP_CHECK(hipMemsetAsync(UmaxSmax, 0, 16, ctx->stream));
        }
        return IMCOM_OK;
    }
    WsPlan plan;
    plan.add(gi_system_bytes(G) + 4096);
    st.plan(plan, {szIn, szM, szOut, szOM});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    GiSystem S;
    IMCOM_TRY(gi_system(ctx, G, samp, Cov, epsilon, S));
    S.P.stest = stest;
    S.P.blocksize = blocksize;
    unsigned long long *um;
    IMCOM_TRY(ws_take(ctx, 2, &um, __func__));
    GiResample R;
    R.nlayer = nlayer; R.ny_in = ny_in; R.nx_in = nx_in; R.nx = nx; R.f64 = in_f64; R.bb = bb;
    R.t00 = transform[0]; R.t01 = transform[1]; R.t10 = transform[2]; R.t11 = transform[3];
    R.o0 = origin[0]; R.o1 = origin[1];
    R.umax_bits = um;
    // (the layers as bytes: float32 or float64)
    const unsigned char *ind;
    unsigned char *outd;
    IMCOM_TRY(st.in((const unsigned char *)in, szIn, &ind));
    IMCOM_TRY(st.in(in_mask, szM, &R.in_mask));
    IMCOM_TRY(st.out((unsigned char *)out, szOut, &outd));
    IMCOM_TRY(st.out(out_mask, szOM, &R.out_mask));
    R.in = ind;
    R.out = outd;
    IMCOM_HIP_CHECK(hipMemsetAsync(um, 0, 16, ctx->stream));
    IMCOM_TRY(gi_launch_tiles(ctx, S, npts, nullptr, nullptr, nullptr, nullptr, nullptr, R));
    IMCOM_TRY(st.back((unsigned char *)out, outd, szOut));
    IMCOM_TRY(st.back(out_mask, R.out_mask, szOM));
    // UmaxSmax: a copy in either memory space (the kernel's maxima are bit patterns in the workspace)
    IMCOM_HIP_CHECK(hipMemcpyAsync(UmaxSmax, um, 16, st.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return st.done();
}

// ------------------------------------------------------------------------------------------------
// The mosaic that the resampler reads (seam 19; reference src/pyimcom/meta/distortimage.py): the input side of this file.  MetaMosaic's
// constructor pastes the windows of up to nine block files into one square (146-207), its mask methods cut on the dB maps (223-280) and
// rasterise circles (340-352).  The entries imcom_mosaic_paste, imcom_mosaic_mask_cut and imcom_mosaic_caps end the file; the index
// maps, the dB arithmetic, the boxes and the predicate are mosaic_core.h's.  Every pointer of these entries is device memory.

namespace {

struct MoPaste {
    MoWindow W;
    int ns, nlayer, es;  // side of the mosaic; layers; bytes of a layer element (4 or 8)
    const unsigned char *primary;
    long layer_stride, row_stride;  // elements
    const void *fid, *sig;          // the coded maps, [by][..] with the row strides below
    int fid_type, sig_type;
    long fid_stride, sig_stride;
    float fid_bels, sig_bels;
    unsigned char *image;
    float *fidelity, *noise;
    unsigned char *mask;
};

template <typename T>
__device__ __forceinline__ void mo_copy_row(const unsigned char *src, unsigned char *dst, int w, int lane)
{
    int lead, nvec;
    mo_row_split((uint64_t)dst, (uint64_t)src, w, (int)sizeof(T), &lead, &nvec);
    constexpr int per = 16 / (int)sizeof(T);
    const T *s = (const T *)src;
    T *d = (T *)dst;
    const uint4 *sv = (const uint4 *)(s + lead);
    uint4 *dv = (uint4 *)(d + lead);
    for (int k = lane; k < nvec; k += 64) dv[k] = sv[k];
    const int tail = lead + nvec * per;  // the scalar edges: [0, lead) and [tail, w)
    for (int k = lane; k < lead + (w - tail); k += 64) {
        const int c = k < lead ? k : tail + (k - lead);
        d[c] = s[c];
    }
}

// One wave a row of the window, four rows a workgroup, the rows strided over gridDim.x; blockIdx.y: a layer, or (= nlayer) the two dB
// maps and the mask.  Layers are moved as integers: bit for bit, NaN payloads included.
__global__ __launch_bounds__(256) void mosaic_paste_kernel(MoPaste P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, plane = blockIdx.y;
    const int h = mo_rows(P.W), w = mo_cols(P.W);
    for (int r = blockIdx.x * 4 + wave; r < h; r += gridDim.x * 4) {
        const long d0 = mo_dst_offset(P.W, r, P.ns);
        if (plane < P.nlayer) {
            const unsigned char *src = P.primary + ((long)plane * P.layer_stride + mo_src_offset(P.W, r, P.row_stride)) * P.es;
            unsigned char *dst = P.image + ((long)plane * P.ns * P.ns + d0) * P.es;
            if (P.es == 4) mo_copy_row<uint32_t>(src, dst, w, lane);
            else mo_copy_row<uint64_t>(src, dst, w, lane);
            continue;
        }
        const long f0 = mo_src_offset(P.W, r, P.fid_stride), s0 = mo_src_offset(P.W, r, P.sig_stride);
        float *fd = P.fidelity + d0, *nd = P.noise + d0;
        unsigned char *md = P.mask + d0;
        // the float32 rows of both maps share their offset within 16 bytes (the entry checks the bases), and there the mask's four bytes are aligned
        int lead, nvec;
        mo_row_split((uint64_t)fd, (uint64_t)fd, w, 4, &lead, &nvec);
        for (int k = lane; k < nvec; k += 64) {
            const int c = lead + 4 * k;
            float f[4], n[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                f[j] = mo_db(mo_code_value(P.fid, P.fid_type, f0 + c + j), P.fid_bels, MO_FIDELITY_DIV);
                n[j] = mo_db(mo_code_value(P.sig, P.sig_type, s0 + c + j), P.sig_bels, MO_NOISE_DIV);
            }
            *(float4 *)(fd + c) = make_float4(f[0], f[1], f[2], f[3]);
            *(float4 *)(nd + c) = make_float4(n[0], n[1], n[2], n[3]);
            *(uchar4 *)(md + c) = make_uchar4(f[0] == 0.0f, f[1] == 0.0f, f[2] == 0.0f, f[3] == 0.0f);
        }
        const int tail = lead + nvec * 4;
        for (int k = lane; k < lead + (w - tail); k += 64) {
            const int c = k < lead ? k : tail + (k - lead);
            const float f = mo_db(mo_code_value(P.fid, P.fid_type, f0 + c), P.fid_bels, MO_FIDELITY_DIV);
            fd[c] = f;
            nd[c] = mo_db(mo_code_value(P.sig, P.sig_type, s0 + c), P.sig_bels, MO_NOISE_DIV);
            md[c] = f == 0.0f;
        }
    }
}

// mask |= map < cut (mode 1) or map > cut (mode 2), and |= extra != 0.  The map's float32 value and the cut are compared as doubles: exact,
// and a NaN compares false.  Four pixels a thread where n allows (the bases are 16-byte aligned), the last n % 4 one by one.
__global__ __launch_bounds__(256) void mosaic_mask_cut_kernel(unsigned char *__restrict__ mask, const float *__restrict__ map, long n, double cut, int mode,
                                                              const unsigned char *__restrict__ extra)
{
    const long n4 = n / 4, stride = (long)gridDim.x * 256;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4 + (n - 4 * n4); q += stride) {
        if (q < n4) {
            uchar4 m = ((const uchar4 *)mask)[q];
            if (mode) {
                const float4 v = ((const float4 *)map)[q];
                if (mode == 1) m.x |= (double)v.x < cut, m.y |= (double)v.y < cut, m.z |= (double)v.z < cut, m.w |= (double)v.w < cut;
                else m.x |= (double)v.x > cut, m.y |= (double)v.y > cut, m.z |= (double)v.z > cut, m.w |= (double)v.w > cut;
            }
            if (extra) {
                const uchar4 e = ((const uchar4 *)extra)[q];
                m.x |= e.x != 0, m.y |= e.y != 0, m.z |= e.z != 0, m.w |= e.w != 0;
            }
            ((uchar4 *)mask)[q] = m;
        } else {
            const long i = 4 * n4 + (q - n4);
            unsigned char m = mask[i];
            if (mode == 1) m |= (double)map[i] < cut;
            if (mode == 2) m |= (double)map[i] > cut;
            if (extra) m |= extra[i] != 0;
            mask[i] = m;
        }
    }
}

// Circles.  The launch shape: the pixels of all boxes, box after box and row-major inside a box, are ONE flat index space; start [n + 1]
// (int64) is its prefix sum.  A workgroup takes MO_CAPS_CHUNK consecutive flat indices at a time (the chunks strided over the grid) and a
// thread every 256th of them, so a box as large as the mosaic is spread over thousands of workgroups, and boxes of a few pixels fill the
// lanes of a wave one behind the other.  The only writes are byte stores of 1: no atomics, the same result for every order of the objects
// and every grid.
constexpr int MO_CAPS_CHUNK = 4096;

__global__ __launch_bounds__(256) void mosaic_caps_box_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ r, long n, int ns,
                                                              MoBox *__restrict__ box, long *__restrict__ start)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const MoBox b = mo_cap_box(x[i], y[i], r[i], ns);
        box[i] = b;
        start[i + 1] = mo_box_pixels(b);  // (the scan below turns the counts into offsets)
    }
}

// One workgroup: start[i + 1] = sum of the counts up to and including object i, start[0] = 0.
__global__ __launch_bounds__(256) void mosaic_caps_scan_kernel(long n, long *__restrict__ start)
{
    __shared__ long part[256];
    __shared__ long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0, start[0] = 0;
    __syncthreads();
    for (long base = 0; base < n; base += 256) {
        const long i = base + t, v = i < n ? start[i + 1] : 0;
        part[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const long a = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += a;
            __syncthreads();
        }
        if (i < n) start[i + 1] = carry + part[t];
        __syncthreads();
        if (t == 255) carry += part[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mosaic_caps_kernel(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ r, long n, int ns,
                                                          const MoBox *__restrict__ box, const long *__restrict__ start, unsigned char *__restrict__ mask)
{
    const long total = start[n];
    for (long c0 = (long)blockIdx.x * MO_CAPS_CHUNK; c0 < total; c0 += (long)gridDim.x * MO_CAPS_CHUNK) {
        long p = c0 + threadIdx.x;
        if (p >= total) continue;
        // the object that holds p: the last i with start[i] <= p (objects with empty boxes are stepped over)
        long lo = 0, hi = n;  // start[lo] <= p < start[hi]
        while (hi - lo > 1) {
            const long mid = (lo + hi) >> 1;
            if (start[mid] <= p) lo = mid;
            else hi = mid;
        }
        long obj = lo, end = start[obj + 1], first = start[obj];
        MoBox b = box[obj];
        double ox = x[obj], oy = y[obj], orad = r[obj];
        const long stop = c0 + MO_CAPS_CHUNK < total ? c0 + MO_CAPS_CHUNK : total;
        for (; p < stop; p += 256) {
            if (p >= end) {
                do {
                    obj++;
                    end = start[obj + 1];
                } while (p >= end);  // (p < total = start[n]: obj stays below n)
                first = start[obj];
                b = box[obj];
                ox = x[obj], oy = y[obj], orad = r[obj];
            }
            int ix, iy;
            mo_box_pixel(b, p - first, &ix, &iy);
            if (mo_cap_hit(ix, iy, ox, oy, orad)) mask[(long)iy * ns + ix] = 1;
        }
    }
}

constexpr int MO_MAX_SIDE = 32768;  // (a box holds fewer than 2^31 pixels)

int mo_code_bytes(int type) { return type == 0 ? 1 : 2; }

}  // namespace

extern "C" int imcom_mosaic_paste(imcom_ctx *ctx, const void *primary, int prim_f64, long layer_stride, long row_stride, int nlayer, int by, int bx,
                                  const void *fid, int fid_type, long fid_stride, double fid_bels, const void *sig, int sig_type, long sig_stride,
                                  double sig_bels, int symin, int symax, int sxmin, int sxmax, int cy, int cx, int ns, void *in_image, float *in_fidelity,
                                  float *in_noise, unsigned char *in_mask)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(primary && fid && sig && in_image && in_fidelity && in_noise && in_mask && (prim_f64 == 0 || prim_f64 == 1), "mosaic_paste: bad arguments");
    IMCOM_REQUIRE(nlayer >= 1 && nlayer <= 1024 && by >= 1 && bx >= 1 && ns >= 1 && ns <= MO_MAX_SIDE && by <= MO_MAX_SIDE && bx <= MO_MAX_SIDE,
                  "mosaic_paste: %d layers, a block file of %d x %d, a mosaic of side %d", nlayer, by, bx, ns);
    IMCOM_REQUIRE(fid_type >= 0 && fid_type <= 2 && sig_type >= 0 && sig_type <= 2, "mosaic_paste: code types %d, %d (0 uint8, 1 uint16, 2 int16)", fid_type, sig_type);
    IMCOM_REQUIRE(row_stride >= bx && layer_stride >= 0 && fid_stride >= bx && sig_stride >= bx, "mosaic_paste: a row stride below the %d columns of the block file", bx);
    MoPaste P;
    P.W = MoWindow{symin, symax, sxmin, sxmax, cy, cx};
    IMCOM_REQUIRE(mo_window_ok(P.W, by, bx, ns), "mosaic_paste: the window [%d:%d, %d:%d] + (%d, %d) leaves the block file (%d x %d) or the mosaic (%d)", symin, symax,
                  sxmin, sxmax, cy, cx, by, bx, ns);
    const int es = prim_f64 ? 8 : 4;
    IMCOM_REQUIRE((uintptr_t)primary % es == 0 && (uintptr_t)in_image % 16 == 0 && (uintptr_t)in_fidelity % 16 == 0 && (uintptr_t)in_noise % 16 == 0 &&
                      (uintptr_t)in_mask % 4 == 0 && (uintptr_t)fid % mo_code_bytes(fid_type) == 0 && (uintptr_t)sig % mo_code_bytes(sig_type) == 0,
                  "mosaic_paste: a misaligned array");
    const int h = mo_rows(P.W), w = mo_cols(P.W);
    if (h == 0 || w == 0) return IMCOM_OK;
    P.ns = ns; P.nlayer = nlayer; P.es = es;
    P.primary = (const unsigned char *)primary; P.layer_stride = layer_stride; P.row_stride = row_stride;
    P.fid = fid; P.sig = sig; P.fid_type = fid_type; P.sig_type = sig_type; P.fid_stride = fid_stride; P.sig_stride = sig_stride;
    P.fid_bels = (float)fid_bels; P.sig_bels = (float)sig_bels;
    P.image = (unsigned char *)in_image; P.fidelity = in_fidelity; P.noise = in_noise; P.mask = in_mask;
    ProfScope ps(ctx, "mosaic");
    hipLaunchKernelGGL(mosaic_paste_kernel, dim3(std::min((h + 3) / 4, 2048), nlayer + 1), dim3(256), 0, ctx->stream, P);
    return check_launch("mosaic_paste_kernel");
}

extern "C" int imcom_mosaic_mask_cut(imcom_ctx *ctx, unsigned char *mask, const float *map, long n, double cut, int mode, const unsigned char *extra)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(mask && n >= 0 && mode >= 0 && mode <= 2 && (mode == 0 || map) && (mode != 0 || extra), "mosaic_mask_cut: bad arguments");
    IMCOM_REQUIRE((uintptr_t)mask % 4 == 0 && (uintptr_t)map % 16 == 0 && (uintptr_t)extra % 4 == 0, "mosaic_mask_cut: a misaligned array");
    if (n == 0) return IMCOM_OK;
    ProfScope ps(ctx, "mosaic");
    hipLaunchKernelGGL(mosaic_mask_cut_kernel, dim3((unsigned)std::min((n / 4 + 3 + 255) / 256, 4096L)), dim3(256), 0, ctx->stream, mask, map, n, cut, mode, extra);
    return check_launch("mosaic_mask_cut_kernel");
}

extern "C" int imcom_mosaic_caps(imcom_ctx *ctx, const double *x, const double *y, const double *r, long n, int ns, unsigned char *mask)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(n >= 0 && n < (1L << 31) && ns >= 1 && ns <= MO_MAX_SIDE && mask && (n == 0 || (x && y && r)), "mosaic_caps: bad arguments");
    if (n == 0) return IMCOM_OK;
    WsPlan plan;
    plan.add((size_t)n * sizeof(MoBox));
    plan.add((size_t)(n + 1) * sizeof(long));
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    MoBox *box;
    long *start;
    IMCOM_TRY(ws_take(ctx, (size_t)n, &box, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n + 1, &start, __func__));
    ProfScope ps(ctx, "mosaic", 3);
    hipLaunchKernelGGL(mosaic_caps_box_kernel, dim3((unsigned)std::min((n + 255) / 256, 2048L)), dim3(256), 0, ctx->stream, x, y, r, n, ns, box, start);
    IMCOM_TRY(check_launch("mosaic_caps_box_kernel"));
    hipLaunchKernelGGL(mosaic_caps_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, n, start);
    IMCOM_TRY(check_launch("mosaic_caps_scan_kernel"));
    hipLaunchKernelGGL(mosaic_caps_kernel, dim3(ctx->cu_count * 8), dim3(256), 0, ctx->stream, x, y, r, n, ns, box, start, mask);
    return check_launch("mosaic_caps_kernel");
}
