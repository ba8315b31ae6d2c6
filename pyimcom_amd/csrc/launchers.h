// launchers.h -- host-side functions, structs and constants that are used from ANOTHER source file than the one that defines them.  What only
// its own file uses (a seam's launch functions, called by the C entries below them) is static there and has no line here.
#pragma once
#include <functional>

#include "common.h"

namespace imcom {

// gemm_f64.hip
int launch_chol_update(imcom_ctx *ctx, const double *A, double *L, int ldn, int k, int nbmax, int batch, int abatch,
                       const int *nblk, const double *dshift, double *partial, int nparts);  // nparts > 1: split-K through `partial`
int launch_chol_trsm(imcom_ctx *ctx, double *L, const double *Dinv, int ldn, int k, int nbmax, int batch,
                     const int *nblk);
int launch_solve_fwd(imcom_ctx *ctx, const double *L, const double *Bt, double *Y, int ldn, int ldm, int k,
                     int batch, int bbatch, const int *nblk, const int *n, const double *Dinv, double *partial, int nparts,
                     double *Dpart);  // Dinv != null: Linv[k] applied in the same launch; Dpart: column sums of Y^2 per block row
// The coaddition sums (coadd.py:1320-1354) riding in the backward launches: per block row and wave row of a tile, the column sums
// sum_j T[j][a] w_q[j] over the tile's rows with w_q = the indicator of exposure q (q < n_expo) or input frame q - n_expo --
// Epart [batch][2 ldn / 128][n_expo + n_inframe][ldm]; launch_coadd_from_partials adds them up in a fixed order.
struct CoaddFuse {
    const float *indata = nullptr;  // [batch][n_inframe][ldn]
    const int *expo = nullptr;      // [batch][ldn]
    int n_inframe = 0, n_expo = 0;
    double *Epart = nullptr;
};
int launch_solve_bwd(imcom_ctx *ctx, const double *L, double *Y, int ldn, int ldm, int k, int nbmax, int batch,
                     const int *nblk, const int *n, const double *Dinv, double *partial, int nparts, double *Npart, float *Tt,
                     const CoaddFuse *cf = nullptr);
int launch_coadd_from_partials(imcom_ctx *ctx, int batch, const int *n_dev, const int *nblk_dev, int ldn, int m, int ldm, int n2, const CoaddFuse &cf,
                               float *outimage, double *Tsum_image, double *Tsum_stamp, double *Tsum_inpix, double *Neff);
int launch_solve_dinv(imcom_ctx *ctx, const double *Dinv, double *Y, int ldn, int ldm, int k, int batch,
                      const int *nblk, bool trans);
int launch_syr2k_lower(imcom_ctx *ctx, int N, int K, int batch, const double *V, long ldv, long strideV, const double *W, long ldw, long strideW,
                       double *C, long ldc, long strideC, double alpha);  // lower 128-tiles of C += alpha (V^T W + W^T V), V, W k-major
int launch_gemm(imcom_ctx *ctx, bool akm, bool bkm, int M, int N, int K, int batch, const double *A, long lda,
                long strideA, const double *B, long ldb, long strideB, double *C, long ldc, long strideC,
                double alpha, double beta);

// tridiag.hip: the tridiagonal QR eigensolver
size_t eigh_ws_bytes(int batch, int ld, bool vectors);
int eigh_device(imcom_ctx *ctx, int batch, const int *n_host, int ld, const double *A, long lda, long strideA, double *lam,
                long ldlam, double *Q, long ldq, long strideQ, int *sweeps_out);

// tridiag.hip: the tridiagonal basis A = Qh T Qh^T without eigenvectors (eigen.hip works in it)
constexpr int BAND_BW = 4;  // bandwidth of band.hip's reduction
struct TrdBasis {
    double *Vall, *dvec, *evec, *tauvec;  // reflectors [batch][ld][ld] (row j = v_j), T's diagonal / off-diagonal, tau [batch][ld]
    double *Tm, *Sm, *W1, *W2;            // triangular factors of the 128-reflector panels [npanels][batch][128][128]; scratch of trd_apply_q
    double *band = nullptr;               // band.hip: [batch][bw + 1][ld], band[t][i] = B[i + t][i]
    double *T2 = nullptr;                 // factors of PAIRS of panels (256 reflectors) [npanels / 2][batch][256][256]; W1, W2 then hold 256 rows
    int *n_dev;
    int ld, nmax, npanels, bw = 1;        // bw: rows between a reflector's column and its pivot (1: tridiagonal basis)
};
size_t trd_basis_ws_bytes(int batch, int ld, int mp);
int trd_basis_device(imcom_ctx *ctx, int batch, const int *n_host, int ld, int mp, const double *A, long lda, long strideA, TrdBasis *out);
int trd_apply_q(imcom_ctx *ctx, const TrdBasis &b, int batch, double *C, int mp, bool transpose);
int trd_pair_factors(imcom_ctx *ctx, TrdBasis *out, int batch);  // T2 from Tm (all panels' factors must be there)
// band.hip: the same with A = Q B Q^T, B of bandwidth BAND_BW (a quarter of the passes over the matrix); ld up to what the panel's LDS holds
bool band_basis_fits(int ld);
size_t band_basis_ws_bytes(int batch, int ld, int mp);
size_t band_basis_keep_bytes(int batch, int ld, int mp);  // the part of it that outlives band_basis_device (reflectors, factors, W1 / W2)
// on_panel(p) (optional) is called on the host as soon as the launches that complete the 128 reflectors of panel p have been queued:
// the caller may start applying them on another stream; the panels' T factors are then the caller's job (trd_panel_step)
int band_basis_device(imcom_ctx *ctx, int batch, const int *n_host, int ld, int mp, const double *A, long lda, long strideA, TrdBasis *out,
                      const std::function<int(int)> &on_panel = nullptr);
int trd_panel_step(imcom_ctx *ctx, const TrdBasis &b, int batch, int p, double *C, int mp);  // T factor of panel p, then C <- (I - V T^T V^T) C (one step of Qh^T C)

// la_kernels.hip
int launch_chol_diag(imcom_ctx *ctx, double *L, double *Dinv, int ldn, int k, int batch, const int *nblk, int *fail);
// chol_diag.hip: T [batch][128][128] of the block reflector of reflectors ps .. ps+127 from S = V V^T [batch][128][128] and tau [batch][ld]
int launch_larft_inv(imcom_ctx *ctx, const double *S, const double *tauvec, int ld, int ps, double *T, int batch);
int launch_diag_shift(imcom_ctx *ctx, const double *A, int ldn, const double *inc, const int *ninc, double *dshift,
                      int batch);
int launch_pack_A(imcom_ctx *ctx, const double *A, long lda, const int *n, double *Ap, int ldp, int batch);
int launch_pack_Bt(imcom_ctx *ctx, const double *B, long ldb, int m, const int *n, double *Bt, int ldp, int ldm,
                   int batch);
int launch_unpack_T(imcom_ctx *ctx, const float *Tt, int ldp, int ldm, const int *n, int m, float *T, long ldt,
                    int batch);
int launch_finalize_fused(imcom_ctx *ctx, const double *Dpart, const double *Npart, int ldn, int ldm, int m, const int *n,
                          const int *nblk, const double *kap, const double *Cs, float *Tt, float *UC, float *Sigma, float *kappa,
                          int batch, const int *act = nullptr);  // act != null: only the stamps with act[s] != 0
int launch_solve_mask(imcom_ctx *ctx, const int *nblk, const int *fac, const int *fail, int *nblk_sol, int *act, int batch);
// lmin_skinny.hip: the smallest-eigenvalue iteration on blocks of 16 vectors [batch][ldn][16] (one workgroup per stamp streams the factor;
// nblk[s] = 0: the stamp is left alone)
constexpr int LMIN_SKINNY_P = 16;
int launch_skinny_solve(imcom_ctx *ctx, const double *L, const double *Dinv, const double *X, double *Y, int ldn, const int *nblk, int batch);  // Y = (L L^T)^-1 X (X may be Y)
int launch_skinny_solve_few(imcom_ctx *ctx, const double *L, const double *Dinv, const double *X, double *Y, int ldn, const int *nblk, int nbmax, int batch,
                            double *partial);  // the same for FEW stamps: two short launches per block row and sweep; partial: skinny_few_partial_doubles(batch) doubles
size_t skinny_few_partial_doubles(int batch);
int launch_skinny_ax(imcom_ctx *ctx, const double *A, const double *X, double *Z, int ldn, const int *nblk, int nbmax, int batch);              // Z = A X
int launch_skinny_orth(imcom_ctx *ctx, const double *src, double *dst, int ldn, const int *nblk, int *fail, int batch);                        // one CholQR pass
int launch_skinny_rr(imcom_ctx *ctx, const double *X, const double *Z, int ldn, const int *nblk, double *lam, double *part, int ngroups, int batch);  // eigenvalues of X^T Z [batch][16], residuals of the two lowest pairs
constexpr int LMIN_RESID_GROUPS = 32;  // row groups of launch_skinny_rr: part is [batch][32][2]
int launch_lmin_init(imcom_ctx *ctx, double *X, int ldn, int P, const int *n, const int *want, int batch);
int launch_diag_max(imcom_ctx *ctx, const double *A, int ldn, const int *n, double *dmax, int batch);
int launch_finalize_single(imcom_ctx *ctx, const double *X, const double *Bt, int ldn, int ldm, int m, const int *n,
                           const double *kap, const double *Cs, float *Tt, float *UC, float *Sigma, float *kappa,
                           int batch, const int *act = nullptr);
int launch_multi(imcom_ctx *ctx, const double *Xs, long node_stride, const double *Bt, int ldn, int ldm, int m,
                 const int *n, int nv, const double *kappaC_dev, const double *Cs, double ucmin, double smax,
                 double *Dp, double *Npq, double *W, float *Tt, float *UC, float *Sigma, float *kappa, int batch);
int launch_build_reduced_T(imcom_ctx *ctx, const double *Nf, const double *Df, const double *Ef, const double *kappa,
                           int nv, long m, double ucmin, double smax, double *ok, double *oS, double *oU, double *ow);
int launch_lakernel1(imcom_ctx *ctx, const double *lam, const double *mPhalf, long m, long n, long ldp, double C,
                     double targetleak, double kCmin, double kCmax, int nbis, double *kappa, double *Sigma,
                     double *UC, double *T, long ldt, double smax);
int launch_epilogue(imcom_ctx *ctx, int batch, const int *n_dev, int ldn, int m, int ldm, int n2f, int fade, int n2,
                    float *Tt, const float *indata, int n_inframe, const int *expo, int n_expo, float *outimage,
                    double *Tsum_image, double *Tsum_stamp, double *Tsum_inpix, double *Neff);

// interp.hip
int launch_grid(imcom_ctx *ctx, const double *infunc, int ngy, int ngx, const double *xpos, const double *ypos,
                long npi, int nxo, int nyo, double *fhatout);

// psf_sample.hip: the device work of imcom_smooth_and_pad on its own (src, dst in device memory), its scratch out of the workspace
struct SmoothPadWs {
    double *I, *Y, *Z, *Cy, *Cx, *ky, *kx;
};
size_t smooth_pad_ws_bytes(int n, int ny, int nx, double tophatwidth, double gaussiansigma);
int smooth_pad_take(imcom_ctx *ctx, int n, int ny, int nx, double tophatwidth, double gaussiansigma, SmoothPadWs *w, const char *who);
int smooth_pad_device(imcom_ctx *ctx, const SmoothPadWs &w, int n, const double *src, int ny, int nx, double tophatwidth, double gaussiansigma,
                      double *dst);

// fft.hip: the host side of the line-transform engine.  For the wave-per-line butterflies (fft_lines.h; the plan is fft_plan_core.h): the
// stage tables of a plan (tw: pl.n complex values, device memory), and the opt-in of a line kernel to more than 48 KiB of dynamic LDS
struct FftPlan;
int fft_line_twiddles(imcom_ctx *ctx, const FftPlan &pl, double2 *tw);
int fft_line_lds_opt_in(const void *kernel, size_t lds_bytes);
// The dense-DFT line engine, for the sides the butterflies do not take: plan / take the DFT matrix (forward, and inverse if asked), the packed
// lines A and the product C; after dft_dense_product row l of d.C (stride d.Np doubles) holds the transform of line l of `in`, interleaved (re, im)
constexpr int DFT_DENSE_MAXN = 4096;  // largest line
struct DftDense {
    int N = 0, Kp = 0, Np = 0;
    long Mp = 0;  // padded line count of the largest batch
    double *Mf = nullptr, *Mi = nullptr, *A = nullptr, *C = nullptr;
};
void dft_dense_plan(DftDense &d, int N, long nlines, bool inverse, WsPlan &plan);
int dft_dense_take(imcom_ctx *ctx, DftDense &d, bool inverse, const char *who);
int dft_dense_product(imcom_ctx *ctx, const DftDense &d, const double2 *in, long nlines, bool inv);

// pcg64.hip: jumps [PCG64_JUMPS][2][2] (device memory), the (low, high) halves of A_j and C_j, the affine map of 2^j steps of numpy's
// PCG64 stream with the increment (inc_lo, inc_hi); pcg64_jumps forms them on the host and puts them into the workspace
constexpr int PCG64_JUMPS = 128;
constexpr long PCG64_MAX_COUNT = 1L << 36;  // most draws of one call
int pcg64_jumps(imcom_ctx *ctx, uint64_t inc_lo, uint64_t inc_hi, const unsigned long long **jumps_d, const char *who);

// poisson.hip: numpy's Poisson draws of a PCG64 stream, for the entries at the end of ziggurat.hip.  pcg64_poisson_plan fills in the
// defaults of S, W, T (0) and the guard band (negative), refuses what is out of range and counts the workspace; pcg64_poisson_device makes
// the draws (every pointer device memory; values or layer; info_h [4]: outputs consumed, undecided, superchunks recovered, invalid rate)
int pcg64_poisson_plan(long count, int *S, int *W, int *T, double *guard, size_t *ws_bytes, size_t *scratch_bytes);
int pcg64_poisson_device(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long inc[2], const unsigned long long offset[2],
                         const double *lam, const double *brightness, double tot_int, double bg, long count, long *values, float *layer, int S, int W, int T,
                         double guard, int force_walk, unsigned long long *info_h, const char *who);

// wcs.hip: what every entry that takes packed descriptors does with them -- the refusals of a descriptor and of an error table's geometry, and
// the rotation product M = R_to R_from^T (row-major, nine doubles) that wcs_pix2pix (wcs_core.h) takes
struct WcsDesc;
int wcs_descriptor(const double *d, const char *who, WcsDesc *out);
int wcs_table_check(const void *tab, int f64, int n2, double lo, double hi, const char *who);
void wcs_rotation_product(const WcsDesc &from, const WcsDesc &to, double *M);
size_t wcs_gain_ws_bytes(int nside);  // the workspace of imcom_wcs_effective_gain (a destripe mosaic plans for it)

// layers.hip: one plane of the input-layer cube for imcom_layer_place (partition.hip) -- src and dst device memory, the arguments checked
// by layer_place_check (layers_core.h), nside >= 1
int launch_layer_place(imcom_ctx *ctx, const void *src, int src_type, int src_swapped, int src_nx, int y0, int x0, int flip, int op, double sub, int post_scale_flag,
                       double scale, float *dst, int nside);

}  // namespace imcom
