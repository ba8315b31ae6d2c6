// destripe.hip -- cost and gradient of the destriping stage (reference src/pyimcom/imdestripe.py): the bilinear gather of every
// neighbour B onto a target SCA A with the stripe parameters subtracted on the way (Sca_img.make_interpolated 476-594,
// subtract_parameters 430-449, apply_all_mask 421-427, Parameters.forward_par 670-703), psi and its cost (cost_function_single
// 1546-1551, 875-887, the boundary penalty 1413-1489) and the transposed scatter of f'(psi) into the parameter bins of every
// neighbour (residual_function_single 1375-1403, transpose_par 1026-1058).  The C-ABI entries imcom_destripe_* end the file.
//
// The interpolation cell (the reference's tests/pyimcom/test_imdestripe.py 173-189, 240-256 on the C routine): positions are
// (x, y) = (column, row) in the source, the cell is floor, a target pixel whose cell is not wholly inside the source contributes
// nothing.  Sums that many threads feed (the parameter bins, the transposed image) are exact: every contribution is rounded once to
// a fixed-point integer of a scale common to the call and added as an integer, so the order of arrival cannot change a bit.
//
// Where a pair's positions come from: two stored arrays, a lattice, or (seam 21) the two WCSs themselves -- wcs_core.h's wcs_pix2pix on
// the integer pixel, the arithmetic of wcs_pix2pix_kernel (wcs.hip) in its order, so the position a kernel forms is the one that kernel
// would have stored, bit for bit.  The descriptors sit in a device table indexed by SCA; a workgroup's pair is one, so every coefficient
// read is wave-uniform.
#include <algorithm>

#include "launchers.h"
#include "wcs_core.h"

namespace imcom {

struct DsPair {            // one ordered pair: neighbour b gathered onto / scattered from target a
    const double *x, *y;   // positions of a's pixels in b [nside][nside] (column, row), or both null:
    const double *lat;     // their values on the lattice [2][L][L] (x plane, y plane; row node, column node), or null as well:
    const double *M;       // R_b R_a^T (nine doubles): the positions are formed from the descriptors and error tables of a and b
    int a, b;
};
struct DsWcs {             // the WCSs of the mosaic, indexed by SCA (null: no pair is formed)
    const WcsDesc *desc;
    const WcsTab *tab;
};
struct DsGeom {
    int n_sca, nside, ds_rows, amp_cols, ncb, nbins;  // ncb column blocks (0: rows only), nbins = ds_rows + ncb
    int L, max_np;                                    // lattice nodes per axis (0: no lattice pair), most neighbours of one target
    int model;
    double thresh, neff_min, lambda;
};

constexpr int DS_T = 256;      // threads of a workgroup
constexpr int DS_ROWS = 8;     // target rows a workgroup of the scatter serves before it flushes its bins

__device__ inline double block_sum(double v, double *red)  // fixed-order tree over the 256 threads; every thread gets the sum
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = DS_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// The position of target pixel (r, c) in the source of a pair: the stored arrays, the tensor product over the lattice with the
// row axis already contracted (T [2][L] in LDS: T[k][j] = sum_i W[r][i] lat[k][i][j]), or wcs_pix2pix of the pixel with the NaN rule
// of wcs_pix2pix_kernel (a point that has no image, or one that is not finite, is NaN: outside every cell).
__device__ inline void pair_position(const DsPair &p, const DsWcs &ws, const double *T, const double *__restrict__ W, int L, int nside, int r, int c, double *x,
                                     double *y)
{
    if (p.x) {
        const long o = (long)r * nside + c;
        *x = p.x[o];
        *y = p.y[o];
        return;
    }
    if (!p.lat) {
        const WcsDesc &from = ws.desc[p.a], &to = ws.desc[p.b];
        double xf = NAN, yf = NAN;
        // (imcom_destripe_pair_rotation refuses a bad descriptor on the host when the pair is registered; the table in device memory is
        // bounded here once more, by a few wave-uniform compares, since the orders are loop bounds over the coefficient blocks)
        const bool sane = from.d[WCS_D_AORDER] <= WCS_MAX_ORDER && from.d[WCS_D_BORDER] <= WCS_MAX_ORDER && to.d[WCS_D_AORDER] <= WCS_MAX_ORDER &&
                          to.d[WCS_D_BORDER] <= WCS_MAX_ORDER && to.d[WCS_D_NITER] <= WCS_MAX_NITER;
        if (!sane || !wcs_pix2pix(from, ws.tab[p.a], to, ws.tab[p.b], p.M, (double)c, (double)r, 0, &xf, &yf) || !(xf - xf == 0.0 && yf - yf == 0.0))
            xf = NAN, yf = NAN;
        *x = xf;
        *y = yf;
        return;
    }
    const double *w = W + (long)c * L;
    double sx = 0.0, sy = 0.0;
    for (int j = 0; j < L; j++) {
        sx = fma(w[j], T[j], sx);
        sy = fma(w[j], T[L + j], sy);
    }
    *x = sx;
    *y = sy;
}

__device__ inline void contract_rows(const DsPair *pairs, int np, const double *__restrict__ W, int L, int r, double *T)
{
    for (int idx = threadIdx.x; idx < np * 2 * L; idx += DS_T) {
        const int q = idx / (2 * L), kj = idx - q * 2 * L;
        double s = 0.0;
        if (!pairs[q].x && pairs[q].lat) {
            const double *lat = pairs[q].lat + kj / L * L * L + kj % L;
            for (int i = 0; i < L; i++) s = fma(W[(long)r * L + i], lat[(long)i * L], s);
        }
        T[idx] = s;
    }
    __syncthreads();
}

// The interpolation cell of position (x, y) in a source of rows x cols and its four bilinear weights, w[2 ky + kx] for the corner
// (y1 + ky, x1 + kx).  False when the cell is not wholly inside (x1 < 0, y1 < 0, x1 + 1 >= cols, y1 + 1 >= rows; written so that a NaN
// position is outside).  Every kernel of this file, the engine's and the two routines on their own, takes its cells from here.
__device__ inline bool bilinear_cell(double x, double y, int rows, int cols, int *x1, int *y1, double *w)
{
    if (!(x >= 0.0 && y >= 0.0 && x < (double)(cols - 1) && y < (double)(rows - 1))) return false;
    *x1 = (int)floor(x), *y1 = (int)floor(y);
    const double dx = x - *x1, dy = y - *y1;
    w[0] = (1.0 - dx) * (1.0 - dy), w[1] = dx * (1.0 - dy), w[2] = (1.0 - dx) * dy, w[3] = dx * dy;
    return true;
}

// the masked, parameter-subtracted pixel of an SCA (430-449, 421-427): NaN -> 0
__device__ inline double destriped(const DsGeom &g, const float *__restrict__ img, const unsigned char *__restrict__ mask, const double *__restrict__ par, int yy,
                                   int xx)
{
    const long o = (long)yy * g.nside + xx;
    double p = par[yy];
    if (g.ncb > 0) p += par[g.ds_rows + xx / g.amp_cols];
    const double v = (double)img[o] - p;
    return v != v ? 0.0 : v * (double)mask[o];
}

__device__ inline double cost_f(double x, int model, double d)
{
    const double a = fabs(x);
    if (model == IMCOM_DESTRIPE_ABSOLUTE) return a;
    if (model == IMCOM_DESTRIPE_HUBER && !(a <= d)) return d * d + 2.0 * d * (a - d);
    return x * x;
}

__device__ inline double cost_fprime(double x, int model, double d)
{
    const double sg = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x);
    if (model == IMCOM_DESTRIPE_ABSOLUTE) return sg;
    if (model == IMCOM_DESTRIPE_HUBER && !(fabs(x) <= d)) return 2.0 * d * sg;
    return 2.0 * x;
}

// One workgroup per (row r of target a).  MODE 0: N_eff[a] = sum_B Interp_{B->A}[mask_B] (535-562).  MODE 1: J_A, psi and the row's
// share of epsilon; I_A is read once, psi written once, every neighbour is gathered in the order of the pair table (ascending b).
template <int MODE>
__global__ __launch_bounds__(DS_T) void destripe_forward_kernel(DsGeom g, const float *__restrict__ img, const unsigned char *__restrict__ mask,
                                                                const float *__restrict__ geff, const double *__restrict__ params,
                                                                const DsPair *__restrict__ pairs, const int *__restrict__ start, const DsWcs ws,
                                                                const double *__restrict__ W, double *__restrict__ neff, float *__restrict__ psi,
                                                                double *__restrict__ eps_rows)
{
    extern __shared__ double Tl[];  // [np][2][L], then 256 doubles of the reduction
    const int r = blockIdx.x, a = blockIdx.y, n = g.nside;
    const long plane = (long)n * n;
    const int p0 = start[a], np = start[a + 1] - p0;
    double *red = Tl + (size_t)g.max_np * 2 * g.L;
    if (g.L > 0) contract_rows(pairs + p0, np, W, g.L, r, Tl);
    double eps = 0.0;
    for (int c = threadIdx.x; c < n; c += DS_T) {
        double J = 0.0;
        for (int q = 0; q < np; q++) {
            const DsPair &p = pairs[p0 + q];
            double x, y;
            pair_position(p, ws, Tl + (size_t)q * 2 * g.L, W, g.L, n, r, c, &x, &y);
            int x1, y1;
            double w[4];
            if (!bilinear_cell(x, y, n, n, &x1, &y1, w)) continue;
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int yy = y1 + (k >> 1), xx = x1 + (k & 1);
                const long o = (long)p.b * plane + (long)yy * n + xx;
                if (MODE == 0)
                    v[k] = (double)mask[o];
                else
                    v[k] = destriped(g, img + (long)p.b * plane, mask + (long)p.b * plane, params + (long)p.b * g.nbins, yy, xx) * (double)geff[o];
            }
            J += w[0] * v[0] + w[1] * v[1] + w[2] * v[2] + w[3] * v[3];
        }
        const long o = (long)a * plane + (long)r * n + c;
        if (MODE == 0) {
            neff[o] = J;
        } else {
            const double ne = neff[o];
            const bool nm = ne > g.neff_min;  // 573-577
            J = nm ? J / ne : 0.0;
            J = J / (double)geff[o];
            const double ia = destriped(g, img + (long)a * plane, mask + (long)a * plane, params + (long)a * g.nbins, r, c);
            const float ps = (nm && mask[o]) ? (float)(ia - J) : 0.0f;  // 1547-1549
            psi[o] = ps;
            eps += cost_f((double)ps, g.model, g.thresh);
        }
    }
    if (MODE == 1) {
        const double s = block_sum(eps, red);
        if (threadIdx.x == 0) eps_rows[(long)a * n + r] = s;
    }
}

// The boundary-continuity penalty (1413-1489): one workgroup per (chunk of 100 rows every 400, boundary b, SCA a): the means of the
// unmasked destriped pixels in the 50 columns either side of column b amp_cols; pen = (left - right)^2 (NaN when a side is empty,
// as np.mean of nothing is).
__global__ __launch_bounds__(DS_T) void destripe_penalty_kernel(DsGeom g, const float *__restrict__ img, const unsigned char *__restrict__ mask,
                                                                const double *__restrict__ params, double *__restrict__ pen)
{
    __shared__ double red[DS_T];
    const int chunk = blockIdx.x, b = blockIdx.y + 1, a = blockIdx.z, n = g.nside;
    const long plane = (long)n * n;
    const int r0 = chunk * 400, r1 = min(r0 + 100, n), cw = 50;
    double s[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0};
    for (int idx = threadIdx.x; idx < (r1 - r0) * 2 * cw; idx += DS_T) {
        const int rr = r0 + idx / (2 * cw), k = idx % (2 * cw), cc = b * g.amp_cols - cw + k, side = k >= cw;
        if (cc < 0 || cc >= n) continue;
        if (mask[(long)a * plane + (long)rr * n + cc]) {
            s[side] += destriped(g, img + (long)a * plane, mask + (long)a * plane, params + (long)a * g.nbins, rr, cc);
            cnt[side] += 1.0;
        }
    }
    const double sl = block_sum(s[0], red), cl = block_sum(cnt[0], red), sr = block_sum(s[1], red), cr = block_sum(cnt[1], red);
    if (threadIdx.x == 0) {
        const double d = sl / cl - sr / cr;
        pen[((long)a * (g.ncb - 1) + (b - 1)) * gridDim.x + chunk] = d * d;
    }
}

// eps[a] = sum_r eps_rows[a][r] + lambda sum pen[a][..] in a fixed order (one workgroup per SCA)
__global__ __launch_bounds__(DS_T) void destripe_eps_kernel(int n, const double *__restrict__ eps_rows, const double *__restrict__ pen, int npen, double lambda,
                                                            double *__restrict__ eps)
{
    __shared__ double red[DS_T];
    const int a = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += DS_T) s += eps_rows[(long)a * n + r];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        double p = 0.0;
        for (int i = 0; i < npen; i++) p += pen[(long)a * npen + i];
        eps[a] = npen > 0 ? s + lambda * p : s;
    }
}

__device__ inline double grad_scaled(const DsGeom &g, float ps, float ge, double ne)  // 1375, 1383-1388
{
    const double gr = cost_fprime((double)ps, g.model, g.thresh);
    return ne != 0.0 ? gr / ((double)ge * ne) : 0.0;
}

// term_1 (1377): one workgroup per (row r, SCA a): the row sum of g = f'(psi), the row's share of every column block
// (rowcb [n_sca][nside][ncb]) and max |g / (g_A N_eff)| for the scale of the scatter (a maximum does not depend on the order).
__global__ __launch_bounds__(DS_T) void destripe_grad_prep_kernel(DsGeom g, const float *__restrict__ psi, const float *__restrict__ geff,
                                                                  const double *__restrict__ neff, double *__restrict__ term1, double *__restrict__ rowcb,
                                                                  unsigned long long *__restrict__ gmax_bits)
{
    extern __shared__ double rowbuf[];  // [nside], then 256
    double *red = rowbuf + g.nside;
    const int r = blockIdx.x, a = blockIdx.y, n = g.nside;
    const long base = ((long)a * n + r) * n;
    double s = 0.0, m = 0.0;
    for (int c = threadIdx.x; c < n; c += DS_T) {
        const float ps = psi[base + c];
        const double gr = cost_fprime((double)ps, g.model, g.thresh);
        rowbuf[c] = gr;
        s += gr;
        m = fmax(m, fabs(grad_scaled(g, ps, geff[base + c], neff[base + c])));
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) term1[(long)a * g.nbins + r] = s;
    for (int b = threadIdx.x; b < g.ncb; b += DS_T) {
        double t = 0.0;
        for (int c = b * g.amp_cols; c < (b + 1) * g.amp_cols; c++) t += rowbuf[c];
        rowcb[((long)a * n + r) * g.ncb + b] = t;
    }
    __syncthreads();
    red[threadIdx.x] = m;  // the workgroup's maximum first: one atomic per workgroup
    __syncthreads();
    for (int st = DS_T / 2; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    m = red[0];
    if (threadIdx.x == 0 && m == m) atomicMax(gmax_bits, (unsigned long long)__double_as_longlong(m));  // non-negative doubles order as their bit patterns
}

// column blocks of term_1: the rows' shares added in row order
__global__ __launch_bounds__(DS_T) void destripe_colblock_kernel(DsGeom g, const double *__restrict__ rowcb, double *__restrict__ term1)
{
    __shared__ double red[DS_T];
    const int b = blockIdx.x, a = blockIdx.y, n = g.nside;
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += DS_T) s += rowcb[((long)a * n + r) * g.ncb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) term1[(long)a * g.nbins + g.ds_rows + b] = s;
}

// scale[0] = 2^e with count * bound < 2^(62 - e): the integer sums cannot overflow; scale[1] = 2^-e
__global__ void destripe_scale_kernel(const unsigned long long *__restrict__ gmax_bits, double factor, double count, double *__restrict__ scale)
{
    const double bound = __longlong_as_double((long long)*gmax_bits) * factor * count;
    int k = 0;
    if (bound > 0.0 && bound < 1e300) frexp(bound, &k);
    const int e = max(-900, min(900, 62 - k));
    scale[0] = ldexp(1.0, e);
    scale[1] = ldexp(1.0, -e);
}

// Add v (fixed point) to bin `key` of an LDS histogram; key < 0: nothing.  When the whole wave feeds one bin (the usual case along a
// row of a mildly rotated pair) the wave adds up first -- integers, so any order gives the same bits.
__device__ inline void hist_add(unsigned long long *hist, int key, long long v)
{
    const int k0 = __builtin_amdgcn_readfirstlane(key);
    if (__all(key == k0)) {
        if (k0 < 0) return;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) atomicAdd(&hist[k0], (unsigned long long)v);
    } else if (key >= 0) {
        atomicAdd(&hist[key], (unsigned long long)v);
    }
}

// term_2 (1392-1403) for one ordered pair per blockIdx.y and DS_ROWS target rows per workgroup: every target pixel is read once
// and its four weighted values, times g_B at the corners, go straight into the row and column-block bins of B.
__global__ __launch_bounds__(DS_T) void destripe_scatter_kernel(DsGeom g, const float *__restrict__ psi, const float *__restrict__ geff,
                                                                const double *__restrict__ neff, const DsPair *__restrict__ pairs, const DsWcs ws,
                                                                const double *__restrict__ W, const double *__restrict__ scale,
                                                                unsigned long long *__restrict__ bins)
{
    extern __shared__ double dyn[];  // T [2][L], then the bins
    const DsPair p = pairs[blockIdx.y];
    const int n = g.nside, a = p.a;
    const long plane = (long)n * n;
    double *T = dyn;
    unsigned long long *hist = (unsigned long long *)(dyn + 2 * g.L);
    for (int i = threadIdx.x; i < g.nbins; i += DS_T) hist[i] = 0ull;
    const double sc = scale[0];
    const float *gb = geff + (long)p.b * plane;
    const int npad = (n + DS_T - 1) / DS_T * DS_T;
    for (int r = blockIdx.x * DS_ROWS; r < min(n, (blockIdx.x + 1) * DS_ROWS); r++) {
        __syncthreads();
        if (g.L > 0) contract_rows(&pairs[blockIdx.y], 1, W, g.L, r, T);
        else __syncthreads();
        for (int c = threadIdx.x; c < npad; c += DS_T) {  // whole waves stay in the loop: hist_add is a wave operation
            int ky0 = -1, ky1 = -1, kc0 = -1, kc1 = -1;
            long long vy0 = 0, vy1 = 0, vc0 = 0, vc1 = 0;
            if (c < n) {
                const long o = (long)a * plane + (long)r * n + c;
                const double gv = grad_scaled(g, psi[o], geff[o], neff[o]);
                double x = NAN, y = NAN;
                if (gv != 0.0) pair_position(p, ws, T, W, g.L, n, r, c, &x, &y);  // (a pixel without a gradient needs no position)
                int x1, y1;
                double w[4];
                if (gv != 0.0 && bilinear_cell(x, y, n, n, &x1, &y1, w)) {
                    const double t00 = w[0] * gv * (double)gb[(long)y1 * n + x1], t01 = w[1] * gv * (double)gb[(long)y1 * n + x1 + 1];
                    const double t10 = w[2] * gv * (double)gb[(long)(y1 + 1) * n + x1], t11 = w[3] * gv * (double)gb[(long)(y1 + 1) * n + x1 + 1];
                    ky0 = y1, ky1 = y1 + 1;
                    vy0 = __double2ll_rn((t00 + t01) * sc), vy1 = __double2ll_rn((t10 + t11) * sc);
                    if (g.ncb > 0) {
                        kc0 = g.ds_rows + x1 / g.amp_cols, kc1 = g.ds_rows + (x1 + 1) / g.amp_cols;
                        if (kc0 == kc1) {
                            vc0 = __double2ll_rn(((t00 + t01) + (t10 + t11)) * sc);
                            kc1 = -1;
                        } else {
                            vc0 = __double2ll_rn((t00 + t10) * sc), vc1 = __double2ll_rn((t01 + t11) * sc);
                        }
                    }
                }
            }
            hist_add(hist, ky0, vy0);
            hist_add(hist, ky1, vy1);
            if (g.ncb > 0) {
                hist_add(hist, kc0, vc0);
                hist_add(hist, kc1, vc1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < g.nbins; i += DS_T)
        if (hist[i]) atomicAdd(&bins[(long)p.b * g.nbins + i], hist[i]);
}

// resids = -term_1 + term_2 (1311-1317), term_2 = the integer bins times 2^-e; the two parts on their own when asked for
__global__ __launch_bounds__(DS_T) void destripe_resids_kernel(long total, const double *__restrict__ term1, const unsigned long long *__restrict__ bins,
                                                               const double *__restrict__ scale, double *__restrict__ resids, double *__restrict__ r1,
                                                               double *__restrict__ r2)
{
    const long i = (long)blockIdx.x * DS_T + threadIdx.x;
    if (i >= total) return;
    const double t2 = (double)(long long)bins[i] * scale[1], t1 = term1[i];
    resids[i] = t2 - t1;
    if (r1) r1[i] = 0.0 - t1;
    if (r2) r2[i] = t2;
}

// ---- the two routines on their own (interpolate_image_bilinear 972-998, transpose_interpolate 1001-1023) -------------------------
__global__ __launch_bounds__(DS_T) void destripe_interp_kernel(const double *__restrict__ src, const double *__restrict__ gsrc, int rows, int cols,
                                                               const double *__restrict__ x, const double *__restrict__ y, long npix, double *__restrict__ out)
{
    const long i = (long)blockIdx.x * DS_T + threadIdx.x;
    if (i >= npix) return;
    int x1, y1;
    double w[4];
    if (!bilinear_cell(x[i], y[i], rows, cols, &x1, &y1, w)) return;
    const long o = (long)y1 * cols + x1;
    out[i] += w[0] * src[o] * gsrc[o] + w[1] * src[o + 1] * gsrc[o + 1] + w[2] * src[o + cols] * gsrc[o + cols] + w[3] * src[o + cols + 1] * gsrc[o + cols + 1];
}

__global__ __launch_bounds__(DS_T) void destripe_absmax_kernel(const double *__restrict__ v, long count, unsigned long long *__restrict__ bits)
{
    double m = 0.0;
    for (long i = (long)blockIdx.x * DS_T + threadIdx.x; i < count; i += (long)gridDim.x * DS_T) m = fmax(m, fabs(v[i]));
    if (m == m) atomicMax(bits, (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(DS_T) void destripe_transpose_kernel(const double *__restrict__ img, const double *__restrict__ x, const double *__restrict__ y,
                                                                  long npix, int rows, int cols, const double *__restrict__ scale,
                                                                  unsigned long long *__restrict__ acc)
{
    const long i = (long)blockIdx.x * DS_T + threadIdx.x;
    if (i >= npix) return;
    const double v = img[i], sc = scale[0];
    int x1, y1;
    double w[4];
    if (v == 0.0 || !bilinear_cell(x[i], y[i], rows, cols, &x1, &y1, w)) return;
    const long o = (long)y1 * cols + x1;
    atomicAdd(&acc[o], (unsigned long long)__double2ll_rn(w[0] * v * sc));
    atomicAdd(&acc[o + 1], (unsigned long long)__double2ll_rn(w[1] * v * sc));
    atomicAdd(&acc[o + cols], (unsigned long long)__double2ll_rn(w[2] * v * sc));
    atomicAdd(&acc[o + cols + 1], (unsigned long long)__double2ll_rn(w[3] * v * sc));
}

__global__ __launch_bounds__(DS_T) void destripe_unscale_kernel(const unsigned long long *__restrict__ acc, long count, const double *__restrict__ scale,
                                                                double *__restrict__ out)
{
    const long i = (long)blockIdx.x * DS_T + threadIdx.x;
    if (i < count) out[i] += (double)(long long)acc[i] * scale[1];
}

// ------------------------------------------------------------------------------------------------------------------------------------
static size_t destripe_forward_lds(const DsGeom &g) { return ((size_t)g.max_np * 2 * g.L + DS_T) * sizeof(double); }
static size_t destripe_prep_lds(const DsGeom &g) { return ((size_t)g.nside + DS_T) * sizeof(double); }
static size_t destripe_scatter_lds(const DsGeom &g) { return ((size_t)2 * g.L + g.nbins) * sizeof(double); }

static int launch_destripe_forward(imcom_ctx *ctx, const DsGeom &g, bool make_neff, const float *img, const unsigned char *mask, const float *geff, const double *params,
                            const DsPair *pairs, const int *start, const DsWcs &ws, const double *W, double *neff, float *psi, double *eps_rows)
{
    ProfScope ps(ctx, make_neff ? "destripe_neff" : "destripe_forward");
    const size_t lds = destripe_forward_lds(g);
    const dim3 grid((unsigned)g.nside, (unsigned)g.n_sca);
    if (make_neff) {
        IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)destripe_forward_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(destripe_forward_kernel<0>, grid, dim3(DS_T), lds, ctx->stream, g, img, mask, geff, params, pairs, start, ws, W, neff, psi, eps_rows);
    } else {
        IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)destripe_forward_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(destripe_forward_kernel<1>, grid, dim3(DS_T), lds, ctx->stream, g, img, mask, geff, params, pairs, start, ws, W, neff, psi, eps_rows);
    }
    return check_launch("destripe_forward_kernel");
}

static int launch_destripe_eps(imcom_ctx *ctx, const DsGeom &g, const float *img, const unsigned char *mask, const double *params, const double *eps_rows, double *pen,
                        int nchunk, double *eps)
{
    ProfScope ps(ctx, "destripe_eps");
    const bool penalty = g.ncb > 1 && g.lambda > 0.0;
    if (penalty) {
        hipLaunchKernelGGL(destripe_penalty_kernel, dim3((unsigned)nchunk, (unsigned)(g.ncb - 1), (unsigned)g.n_sca), dim3(DS_T), 0, ctx->stream, g, img, mask,
                           params, pen);
        IMCOM_TRY(check_launch("destripe_penalty_kernel"));
    }
    hipLaunchKernelGGL(destripe_eps_kernel, dim3((unsigned)g.n_sca), dim3(DS_T), 0, ctx->stream, g.nside, eps_rows, (const double *)pen,
                       penalty ? nchunk * (g.ncb - 1) : 0, g.lambda, eps);
    return check_launch("destripe_eps_kernel");
}

static int launch_destripe_gradient(imcom_ctx *ctx, const DsGeom &g, const float *psi, const float *geff, const double *neff, const DsPair *pairs, int npairs,
                             const DsWcs &ws, const double *W, double gmax_all, double *term1, double *rowcb, unsigned long long *gmax_bits, double *scale,
                             unsigned long long *bins, double *resids, double *r1, double *r2)
{
    ProfScope ps(ctx, "destripe_gradient", 5);
    const long total = (long)g.n_sca * g.nbins;
    IMCOM_HIP_CHECK(hipMemsetAsync(gmax_bits, 0, sizeof(unsigned long long), ctx->stream));
    IMCOM_HIP_CHECK(hipMemsetAsync(bins, 0, (size_t)total * sizeof(unsigned long long), ctx->stream));
    size_t lds = destripe_prep_lds(g);
    IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)destripe_grad_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(destripe_grad_prep_kernel, dim3((unsigned)g.nside, (unsigned)g.n_sca), dim3(DS_T), lds, ctx->stream, g, psi, geff, neff, term1, rowcb,
                       gmax_bits);
    IMCOM_TRY(check_launch("destripe_grad_prep_kernel"));
    if (g.ncb > 0) {
        hipLaunchKernelGGL(destripe_colblock_kernel, dim3((unsigned)g.ncb, (unsigned)g.n_sca), dim3(DS_T), 0, ctx->stream, g, (const double *)rowcb, term1);
        IMCOM_TRY(check_launch("destripe_colblock_kernel"));
    }
    hipLaunchKernelGGL(destripe_scale_kernel, dim3(1), dim3(1), 0, ctx->stream, (const unsigned long long *)gmax_bits, gmax_all,
                       (double)g.n_sca * (double)g.nside * (double)g.nside, scale);
    IMCOM_TRY(check_launch("destripe_scale_kernel"));
    if (npairs > 0) {
        lds = destripe_scatter_lds(g);
        IMCOM_HIP_CHECK(hipFuncSetAttribute((const void *)destripe_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(destripe_scatter_kernel, dim3((unsigned)((g.nside + DS_ROWS - 1) / DS_ROWS), (unsigned)npairs), dim3(DS_T), lds, ctx->stream, g, psi,
                           geff, neff, pairs, ws, W, (const double *)scale, bins);
        IMCOM_TRY(check_launch("destripe_scatter_kernel"));
    }
    hipLaunchKernelGGL(destripe_resids_kernel, dim3((unsigned)((total + DS_T - 1) / DS_T)), dim3(DS_T), 0, ctx->stream, total, (const double *)term1,
                       (const unsigned long long *)bins, (const double *)scale, resids, r1, r2);
    return check_launch("destripe_resids_kernel");
}

static int launch_destripe_interp(imcom_ctx *ctx, const double *src, const double *gsrc, int rows, int cols, const double *x, const double *y, long npix, double *out)
{
    ProfScope ps(ctx, "destripe_interp");
    hipLaunchKernelGGL(destripe_interp_kernel, dim3((unsigned)((npix + DS_T - 1) / DS_T)), dim3(DS_T), 0, ctx->stream, src, gsrc, rows, cols, x, y, npix, out);
    return check_launch("destripe_interp_kernel");
}

static int launch_destripe_transpose(imcom_ctx *ctx, const double *img, const double *x, const double *y, long npix, int rows, int cols, unsigned long long *acc,
                              unsigned long long *bits, double *scale, double *out)
{
    ProfScope ps(ctx, "destripe_transpose", 4);
    const long count = (long)rows * cols;
    IMCOM_HIP_CHECK(hipMemsetAsync(bits, 0, sizeof(unsigned long long), ctx->stream));
    IMCOM_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)count * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(destripe_absmax_kernel, dim3((unsigned)std::min<long>((npix + DS_T - 1) / DS_T, 1024)), dim3(DS_T), 0, ctx->stream, img, npix, bits);
    IMCOM_TRY(check_launch("destripe_absmax_kernel"));
    hipLaunchKernelGGL(destripe_scale_kernel, dim3(1), dim3(1), 0, ctx->stream, (const unsigned long long *)bits, 1.0, (double)npix, scale);
    IMCOM_TRY(check_launch("destripe_scale_kernel"));
    hipLaunchKernelGGL(destripe_transpose_kernel, dim3((unsigned)((npix + DS_T - 1) / DS_T)), dim3(DS_T), 0, ctx->stream, img, x, y, npix, rows, cols,
                       (const double *)scale, acc);
    IMCOM_TRY(check_launch("destripe_transpose_kernel"));
    hipLaunchKernelGGL(destripe_unscale_kernel, dim3((unsigned)((count + DS_T - 1) / DS_T)), dim3(DS_T), 0, ctx->stream, (const unsigned long long *)acc, count,
                       (const double *)scale, out);
    return check_launch("destripe_unscale_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: destriping: cost and gradient over a resident mosaic

namespace {
using namespace imcom;

int destripe_geom(int n_sca, int nside, int ds_rows, int amp_cols, int L, int max_np, DsGeom *g)
{
    IMCOM_REQUIRE(n_sca >= 1 && n_sca <= 65535 && nside >= 2 && nside <= 32768 && max_np >= 0, "destripe: %d SCAs of side %d", n_sca, nside);
    if (ds_rows != nside) {
        set_error("destripe: ds_rows=%d, the SCA has %d rows (forward_par, imdestripe.py:690-703, broadcasts one parameter per image row)", ds_rows, nside);
        return IMCOM_ERR_UNSUPPORTED;
    }
    if (amp_cols > 0 && nside % amp_cols != 0) {
        set_error("destripe: amp_cols=%d does not divide the %d image columns (imdestripe.py:643-648)", amp_cols, nside);
        return IMCOM_ERR_UNSUPPORTED;
    }
    if (L != 0 && (L < 2 || L > 33)) {
        set_error("destripe: a lattice of %d nodes per axis (2 <= L <= 33)", L);
        return IMCOM_ERR_UNSUPPORTED;
    }
    g->n_sca = n_sca, g->nside = nside, g->ds_rows = ds_rows, g->amp_cols = amp_cols > 0 ? amp_cols : 0;
    g->ncb = amp_cols > 0 ? nside / amp_cols : 0, g->nbins = ds_rows + g->ncb, g->L = L, g->max_np = max_np;
    g->model = IMCOM_DESTRIPE_QUADRATIC, g->thresh = 0.0, g->neff_min = 0.5, g->lambda = 0.0;
    if (destripe_forward_lds(*g) > 65536 || destripe_prep_lds(*g) > 65536 || destripe_scatter_lds(*g) > 65536) {
        set_error("destripe: side %d with %d bins and %d neighbours of one SCA is beyond what a workgroup's LDS holds", nside, g->nbins, max_np);
        return IMCOM_ERR_UNSUPPORTED;
    }
    return IMCOM_OK;
}

int destripe_model(int model, double thresh, DsGeom *g)
{
    IMCOM_REQUIRE(model == IMCOM_DESTRIPE_QUADRATIC || model == IMCOM_DESTRIPE_ABSOLUTE || model == IMCOM_DESTRIPE_HUBER, "destripe: cost model %d", model);
    IMCOM_REQUIRE(model != IMCOM_DESTRIPE_HUBER || thresh == thresh, "destripe: huber_loss needs a threshold");
    g->model = model, g->thresh = thresh;
    return IMCOM_OK;
}

// the pair table: sorted by (a, b), no pair twice, a != b; *max_np = the most neighbours of one target
int destripe_check_pairs(int n_sca, int L, int npairs, const int *pa, const int *pb, const void *const *px, const void *const *py, const void *const *pl,
                         bool wcs, int *max_np, int *nformed)
{
    IMCOM_REQUIRE(npairs >= 0 && (npairs == 0 || (pa && pb && px && py && pl)), "destripe: null pair table");
    int run = 0;
    *max_np = 0, *nformed = 0;
    for (int i = 0; i < npairs; i++) {
        IMCOM_REQUIRE(pa[i] >= 0 && pa[i] < n_sca && pb[i] >= 0 && pb[i] < n_sca && pa[i] != pb[i], "destripe: pair %d is (%d, %d) of %d SCAs", i, pa[i], pb[i], n_sca);
        IMCOM_REQUIRE(i == 0 || pa[i] > pa[i - 1] || (pa[i] == pa[i - 1] && pb[i] > pb[i - 1]), "destripe: the pair table is not sorted by (a, b) at %d", i);
        IMCOM_REQUIRE((px[i] && py[i]) || (!px[i] && !py[i] && ((pl[i] && L >= 2) || (!pl[i] && wcs))),
                      "destripe: pair %d has neither position arrays nor a lattice, and there is no WCS table to form its positions from", i);
        if (!px[i] && !pl[i]) ++*nformed;
        run = (i > 0 && pa[i] == pa[i - 1]) ? run + 1 : 1;
        if (run > *max_np) *max_np = run;
    }
    return IMCOM_OK;
}

// The WCS arguments of the three entries: wcs_desc [n_sca][WCS_DESC_LEN] and pair_M [npairs][9] in device memory (the row of a pair that is
// not formed is not read), and the error tables as host arrays indexed by SCA (tab[s] a device pointer or null; all five null: no tables).
struct DsWcsArgs {
    const double *desc, *M;
    const void *const *tab;
    const int *f64, *n2;
    const double *lo, *hi;
};

int destripe_upload_pairs(imcom_ctx *ctx, int n_sca, int npairs, const int *pa, const int *pb, const void *const *px, const void *const *py,
                          const void *const *pl, const DsWcsArgs &wa, int nformed, DsPair **pairs_d, int **start_d, DsWcs *ws, const char *who)
{
    std::vector<DsPair> tab((size_t)std::max(npairs, 1));
    std::vector<int> start((size_t)n_sca + 1, 0);
    for (int i = 0; i < npairs; i++) {
        tab[i].x = (const double *)px[i], tab[i].y = (const double *)py[i], tab[i].lat = (const double *)pl[i], tab[i].a = pa[i], tab[i].b = pb[i];
        tab[i].M = (!px[i] && !pl[i]) ? wa.M + (size_t)9 * i : nullptr;
        start[pa[i] + 1]++;
    }
    for (int a = 0; a < n_sca; a++) start[a + 1] += start[a];
    IMCOM_TRY(ws_take(ctx, tab.size(), pairs_d, who));
    IMCOM_TRY(ws_take(ctx, start.size(), start_d, who));
    IMCOM_TRY(upload(ctx, *pairs_d, tab.data(), tab.size()));
    IMCOM_TRY(upload(ctx, *start_d, start.data(), start.size()));
    *ws = DsWcs{nullptr, nullptr};
    if (nformed == 0) return IMCOM_OK;
    IMCOM_REQUIRE(wa.desc && wa.M && ((uintptr_t)wa.desc & 7) == 0 && ((uintptr_t)wa.M & 7) == 0, "%s: formed pairs need the descriptor table and the rotation products", who);
    const bool tables = wa.tab != nullptr;
    IMCOM_REQUIRE(tables == (wa.f64 != nullptr) && tables == (wa.n2 != nullptr) && tables == (wa.lo != nullptr) && tables == (wa.hi != nullptr),
                  "%s: the five arrays of the error tables are given together", who);
    std::vector<WcsTab> wt((size_t)n_sca, WcsTab{nullptr, 0, 0, 0.0, 0.0});
    for (int s = 0; tables && s < n_sca; s++) {
        if (!wa.tab[s]) continue;
        IMCOM_TRY(wcs_table_check(wa.tab[s], wa.f64[s], wa.n2[s], wa.lo[s], wa.hi[s], who));
        wt[s] = WcsTab{wa.tab[s], wa.f64[s] ? 1 : 0, wa.n2[s], wa.lo[s], wa.hi[s]};
    }
    WcsTab *wt_d;
    IMCOM_TRY(ws_take(ctx, wt.size(), &wt_d, who));
    IMCOM_TRY(upload(ctx, wt_d, wt.data(), wt.size()));
    *ws = DsWcs{(const WcsDesc *)wa.desc, wt_d};
    return IMCOM_OK;
}

size_t destripe_cost_ws(const DsGeom &g, int npairs, bool forward)
{
    WsPlan plan;
    plan.add((size_t)std::max(npairs, 1) * sizeof(DsPair));
    plan.add(((size_t)g.n_sca + 1) * sizeof(int));
    plan.add((size_t)g.n_sca * sizeof(WcsTab));
    if (forward) {
        plan.add((size_t)g.n_sca * g.nside * 8);
        plan.add((size_t)g.n_sca * std::max(g.ncb - 1, 1) * ((g.nside + 399) / 400) * 8);
    }
    return plan.total;
}

size_t destripe_resid_ws(const DsGeom &g, int npairs)
{
    WsPlan plan;
    plan.add((size_t)std::max(npairs, 1) * sizeof(DsPair));
    plan.add(((size_t)g.n_sca + 1) * sizeof(int));
    plan.add((size_t)g.n_sca * sizeof(WcsTab));
    plan.add((size_t)g.n_sca * g.nbins * 8);
    plan.add((size_t)g.n_sca * g.nside * std::max(g.ncb, 1) * 8);
    plan.add(8);
    plan.add(16);
    plan.add((size_t)g.n_sca * g.nbins * 8);
    return plan.total;
}
}  // namespace

extern "C" {

int imcom_destripe_sizes(int n_sca, int nside, int ds_rows, int amp_cols, int L, int max_np, int npairs, long *out)
{
    IMCOM_REQUIRE(out && npairs >= 0, "null out");
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, ds_rows, amp_cols, L, max_np, &g));
    const long px = (long)nside * nside;
    out[0] = g.nbins;
    out[1] = g.ncb;
    out[2] = px * (4 + 1 + 4 + 8 + 4);  // image, mask, g_eff, N_eff, psi
    out[3] = px * 16;
    out[4] = (long)L * L * 16;
    out[5] = (long)destripe_cost_ws(g, npairs, true);
    out[6] = (long)destripe_resid_ws(g, npairs);
    out[7] = (long)nside * L * 8;  // the lattice weights W
    return IMCOM_OK;
}

int imcom_destripe_neff(imcom_ctx *ctx, int n_sca, int nside, int L, const unsigned char *mask, int npairs, const int *pair_a, const int *pair_b,
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, double *neff,
                        const double *wcs_desc, const void *const *tab, const int *tab_f64, const int *tab_n2, const double *tab_lo, const double *tab_hi,
                        const double *pair_M)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(mask && neff && (L == 0 || W), "null pointer");
    int max_np, nformed;
    const DsWcsArgs wa = {wcs_desc, pair_M, tab, tab_f64, tab_n2, tab_lo, tab_hi};
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wcs_desc && pair_M, &max_np, &nformed));
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, nside, 0, L, max_np, &g));
    IMCOM_TRY(ws_reserve(ctx, destripe_cost_ws(g, npairs, false)));
    DsPair *pairs_d;
    int *start_d;
    DsWcs ws;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wa, nformed, &pairs_d, &start_d, &ws, __func__));
    return launch_destripe_forward(ctx, g, true, nullptr, mask, nullptr, nullptr, pairs_d, start_d, ws, W, neff, nullptr, nullptr);
}

int imcom_destripe_cost(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *image, const unsigned char *mask,
                        const float *geff, const double *neff, const double *params, int npairs, const int *pair_a, const int *pair_b,
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, int model, double thresh,
                        double neff_min, double col_boundary_const, float *psi, double *eps, const double *wcs_desc, const void *const *tab, const int *tab_f64,
                        const int *tab_n2, const double *tab_lo, const double *tab_hi, const double *pair_M)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && mask && geff && neff && params && psi && eps && (L == 0 || W), "null pointer");
    int max_np, nformed;
    const DsWcsArgs wa = {wcs_desc, pair_M, tab, tab_f64, tab_n2, tab_lo, tab_hi};
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wcs_desc && pair_M, &max_np, &nformed));
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, ds_rows, amp_cols, L, max_np, &g));
    IMCOM_TRY(destripe_model(model, thresh, &g));
    g.neff_min = neff_min, g.lambda = col_boundary_const;
    if (g.ncb > 1 && g.lambda > 0.0 && g.amp_cols < 50) {
        set_error("destripe: the boundary penalty reads 50 columns either side of a boundary, amp_cols=%d", g.amp_cols);
        return IMCOM_ERR_UNSUPPORTED;
    }
    IMCOM_TRY(ws_reserve(ctx, destripe_cost_ws(g, npairs, true)));
    DsPair *pairs_d;
    int *start_d;
    DsWcs ws;
    double *eps_rows, *pen;
    const int nchunk = (nside + 399) / 400;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wa, nformed, &pairs_d, &start_d, &ws, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * nside, &eps_rows, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * std::max(g.ncb - 1, 1) * nchunk, &pen, __func__));
    IMCOM_TRY(launch_destripe_forward(ctx, g, false, image, mask, geff, params, pairs_d, start_d, ws, W, (double *)neff, psi, eps_rows));
    return launch_destripe_eps(ctx, g, image, mask, params, eps_rows, pen, nchunk, eps);
}

int imcom_destripe_residual(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *psi, const float *geff, const double *neff,
                            int npairs, const int *pair_a, const int *pair_b, const void *const *pair_x, const void *const *pair_y,
                            const void *const *pair_lat, const double *W, int model, double thresh, double geff_max, double *resids, double *resids1,
                            double *resids2, const double *wcs_desc, const void *const *tab, const int *tab_f64, const int *tab_n2, const double *tab_lo,
                            const double *tab_hi, const double *pair_M)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(psi && geff && neff && resids && (L == 0 || W), "null pointer");
    IMCOM_REQUIRE(geff_max >= 0.0 && geff_max < 1e300, "destripe: geff_max = %g", geff_max);
    int max_np, nformed;
    const DsWcsArgs wa = {wcs_desc, pair_M, tab, tab_f64, tab_n2, tab_lo, tab_hi};
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wcs_desc && pair_M, &max_np, &nformed));
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, ds_rows, amp_cols, L, max_np, &g));
    IMCOM_TRY(destripe_model(model, thresh, &g));
    IMCOM_TRY(ws_reserve(ctx, destripe_resid_ws(g, npairs)));
    DsPair *pairs_d;
    int *start_d;
    DsWcs ws;
    double *term1, *rowcb, *scale;
    unsigned long long *bits, *bins;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, wa, nformed, &pairs_d, &start_d, &ws, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * g.nbins, &term1, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * nside * std::max(g.ncb, 1), &rowcb, __func__));
    IMCOM_TRY(ws_take(ctx, 1, &bits, __func__));
    IMCOM_TRY(ws_take(ctx, 2, &scale, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * g.nbins, &bins, __func__));
    return launch_destripe_gradient(ctx, g, psi, geff, neff, pairs_d, npairs, ws, W, geff_max, term1, rowcb, bits, scale, bins, resids, resids1, resids2);
}

int imcom_destripe_interp(imcom_ctx *ctx, const double *src, const double *gsrc, int rows, int cols, const double *x, const double *y, long npix, double *out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(src && gsrc && x && y && out && rows >= 2 && cols >= 2 && npix >= 0, "destripe: bad arguments of the interpolation");
    if (npix == 0) return IMCOM_OK;
    return launch_destripe_interp(ctx, src, gsrc, rows, cols, x, y, npix, out);
}

int imcom_destripe_interp_transpose(imcom_ctx *ctx, const double *image, const double *x, const double *y, long npix, int rows, int cols, double *out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && x && y && out && rows >= 2 && cols >= 2 && npix >= 0, "destripe: bad arguments of the transposed interpolation");
    if (npix == 0) return IMCOM_OK;
    WsPlan plan;
    plan.add((size_t)rows * cols * 8);
    plan.add(8);
    plan.add(16);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *acc, *bits;
    double *scale;
    IMCOM_TRY(ws_take(ctx, (size_t)rows * cols, &acc, __func__));
    IMCOM_TRY(ws_take(ctx, 1, &bits, __func__));
    IMCOM_TRY(ws_take(ctx, 2, &scale, __func__));
    return launch_destripe_transpose(ctx, image, x, y, npix, rows, cols, acc, bits, scale, out);
}

// Seam 21: what a mosaic whose pairs are formed from its WCSs keeps on the device, exactly.  out[0]: bytes of one formed pair (its rotation
// product); out[1]: bytes of the descriptor table of n_sca SCAs; out[2]: doubles of one descriptor; out[3]: the workspace that making the
// gain of one SCA of this side takes (imcom_wcs_effective_gain; a peak during set-up).  The error tables are the caller's.
int imcom_destripe_wcs_sizes(int n_sca, int nside, long *out)
{
    IMCOM_REQUIRE(out && n_sca >= 0 && nside >= 1 && nside <= 32768, "destripe_wcs_sizes: %d SCAs of side %d", n_sca, nside);
    out[0] = 9 * sizeof(double);
    out[1] = (long)n_sca * (long)sizeof(WcsDesc);
    out[2] = WCS_DESC_LEN;
    out[3] = (long)wcs_gain_ws_bytes(nside);
    return IMCOM_OK;
}

// M [9] = R_ref R_target^T of two packed descriptors (host memory), after their refusals: the rotation product wcs_pix2pix takes, formed
// where imcom_wcs_pix2pix forms it, so that a formed pair and a stored one start from the same nine numbers.
int imcom_destripe_pair_rotation(const double *target, const double *ref, double *M)
{
    IMCOM_REQUIRE(M, "destripe_pair_rotation: null output");
    WcsDesc wt, wr;
    IMCOM_TRY(wcs_descriptor(target, "destripe_pair_rotation", &wt));
    IMCOM_TRY(wcs_descriptor(ref, "destripe_pair_rotation", &wr));
    wcs_rotation_product(wt, wr, M);
    return IMCOM_OK;
}

}  // extern "C"
