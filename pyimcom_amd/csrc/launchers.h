// launchers.h -- host-side launch functions implemented next to their kernels.
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
int launch_probe_fill(imcom_ctx *ctx, double *p, long count, unsigned seed);
int launch_mfma_probe(imcom_ctx *ctx, int nwg, int iters, double *sink, int *waves_per_wg);
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
int launch_trapezoid_f32(imcom_ctx *ctx, float *maps, long nmaps, int n2f, int fade);
int launch_clamp_min_f32(imcom_ctx *ctx, float *maps, long count, float lo);
int launch_epilogue(imcom_ctx *ctx, int batch, const int *n_dev, int ldn, int m, int ldm, int n2f, int fade, int n2,
                    float *Tt, const float *indata, int n_inframe, const int *expo, int n_expo, float *outimage,
                    double *Tsum_image, double *Tsum_stamp, double *Tsum_inpix, double *Neff);

// interp.hip
int launch_getw(imcom_ctx *ctx, const double *fh, long n, double *w);
int launch_interp(imcom_ctx *ctx, const double *infunc, int nlayer, int ngy, int ngx, const double *xpos,
                  const double *ypos, long nout, double *fhatout, int sym);
int launch_grid(imcom_ctx *ctx, const double *infunc, int ngy, int ngx, const double *xpos, const double *ypos,
                long npi, int nxo, int nyo, double *fhatout);
int launch_build_A(imcom_ctx *ctx, int batch, const int *n_dev, int ldn, const double *x, const double *y,
                   const int *psf, const double *tables, int ntab, int ng, double nc, double dscale,
                   const int *pair_tab, const double *pair_pen, int npsf_max, double *A);
int launch_build_B(imcom_ctx *ctx, int batch, const int *n_dev, int ldn, const double *x, const double *y,
                   const int *psf, const double *tables, int ng, double nc, double dscale, const int *io_tab,
                   int npsf_max, const double *out_x0, const double *out_y0, int n2f, int ldm, double *Bt);


// psf_sample.hip: the device work of imcom_smooth_and_pad on its own (src, dst in device memory), its scratch out of the workspace
struct SmoothPadWs {
    double *I, *Y, *Z, *Cy, *Cx, *ky, *kx;
};
size_t smooth_pad_ws_bytes(int n, int ny, int nx, double tophatwidth, double gaussiansigma);
int smooth_pad_take(imcom_ctx *ctx, int n, int ny, int nx, double tophatwidth, double gaussiansigma, SmoothPadWs *w, const char *who);
int smooth_pad_device(imcom_ctx *ctx, const SmoothPadWs &w, int n, const double *src, int ny, int nx, double tophatwidth, double gaussiansigma,
                      double *dst);

// inject.hip
int launch_cube_contract(imcom_ctx *ctx, const double *planes, int na, long npix, const double *lpoly, int nstar, double scale, double *out);
int launch_draw_stars(imcom_ctx *ctx, int nstar, const double *psfs, int py, int px, const double *xsca, const double *ysca, double oversamp,
                      int d, int nside, double *image);

// imsubtract.hip
int launch_imsub_prepare(imcom_ctx *ctx, const float *K, int ax, int s, int Nl, double *Kf);
int launch_imsub_convolve(imcom_ctx *ctx, const float *canvas, int A, long crow0, long crows, const float *leg, const double *Kf, int ax, int Nl, int s,
                          int nside, int first, int y0, int ny, float *image, double *kh);
int launch_imsub_canvas_add(imcom_ctx *ctx, float *canvas, int A, const double *H, int hh, int hw, const float *area, int s, int row0, int col0);

// destripe.hip
struct DsPair {            // one ordered pair: neighbour b gathered onto / scattered from target a
    const double *x, *y;   // positions of a's pixels in b [nside][nside] (column, row), or both null:
    const double *lat;     // their values on the lattice [2][L][L] (x plane, y plane; row node, column node)
    int a, b;
};
struct DsGeom {
    int n_sca, nside, ds_rows, amp_cols, ncb, nbins;  // ncb column blocks (0: rows only), nbins = ds_rows + ncb
    int L, max_np;                                    // lattice nodes per axis (0: no lattice pair), most neighbours of one target
    int model;
    double thresh, neff_min, lambda;
};
size_t destripe_forward_lds(const DsGeom &g);
size_t destripe_prep_lds(const DsGeom &g);
size_t destripe_scatter_lds(const DsGeom &g);
int launch_destripe_forward(imcom_ctx *ctx, const DsGeom &g, bool make_neff, const float *img, const unsigned char *mask, const float *geff, const double *params,
                            const DsPair *pairs, const int *start, const double *W, double *neff, float *psi, double *eps_rows);
int launch_destripe_eps(imcom_ctx *ctx, const DsGeom &g, const float *img, const unsigned char *mask, const double *params, const double *eps_rows, double *pen,
                        int nchunk, double *eps);
int launch_destripe_gradient(imcom_ctx *ctx, const DsGeom &g, const float *psi, const float *geff, const double *neff, const DsPair *pairs, int npairs,
                             const double *W, double gmax_all, double *term1, double *rowcb, unsigned long long *gmax_bits, double *scale,
                             unsigned long long *bins, double *resids, double *r1, double *r2);
int launch_destripe_interp(imcom_ctx *ctx, const double *src, const double *gsrc, int rows, int cols, const double *x, const double *y, long npix, double *out);
int launch_destripe_transpose(imcom_ctx *ctx, const double *img, const double *x, const double *y, long npix, int rows, int cols, unsigned long long *acc,
                              unsigned long long *bits, double *scale, double *out);


// psf_overlap.hip: the plan of the wave-per-line transforms (fft_lines.h) and its stage tables (tw: pl.n complex values, device memory)
struct FftPlan;
bool fft_line_plan(int n, FftPlan *pl);
int fft_line_twiddles(imcom_ctx *ctx, const FftPlan &pl, double2 *tw);

// splitpsf.hip
constexpr int SPLITPSF_MAXN = 4096;  // largest transform side (2 x the cube side)
constexpr int SPLITPSF_ROUTE_NONE = 0, SPLITPSF_ROUTE_LINES = 1, SPLITPSF_ROUTE_DENSE = 2;
int splitpsf_route(int nfft);
int splitpsf_tophat_npad(double width);
size_t splitpsf_tophat_ws(int nplane, int n, double width);
int launch_splitpsf_tophat(imcom_ctx *ctx, const double *cube, int nplane, int n, double width, double *out);
int launch_splitpsf_split(imcom_ctx *ctx, const double *cube, int npoly, int n, int ns, double r1, double r2, const double *trunc_dev, double *smallpsf,
                          double *resid);
size_t splitpsf_points_ws(int n, int nsca, int npts, bool own_kreal);
int launch_splitpsf_points(imcom_ctx *ctx, const double *resid, int nsca, int npoly, int n, int i0, int npts, const double *lpw, const double *wg,
                           const double *cov, double eps, double *KL, double *K_real, double *zeta, double *zmax);
// its dense-DFT line engine (route 2) for other callers: plan / take the DFT matrix (forward, and inverse if asked), the packed lines A and
// the product C; after splitpsf_dense_product row l of d.C (stride d.Np doubles) holds the transform of line l of `in`, interleaved (re, im)
struct SpDense {
    int N = 0, Kp = 0, Np = 0;
    long Mp = 0;  // padded line count of the largest batch
    double *Mf = nullptr, *Mi = nullptr, *A = nullptr, *C = nullptr;
};
void splitpsf_dense_plan(SpDense &d, int N, long nlines, bool inverse, WsPlan &plan);
int splitpsf_dense_take(imcom_ctx *ctx, SpDense &d, bool inverse, const char *who);
int splitpsf_dense_product(imcom_ctx *ctx, const SpDense &d, const double2 *in, long nlines, bool inv);

// noisespec.hip: noise power spectra of coadded frames
constexpr int NOISEPS_ROUTE_NONE = 0, NOISEPS_ROUTE_LINES = 1, NOISEPS_ROUTE_DENSE = 2, NOISEPS_ROUTE_TWOLEVEL = 3;
int noiseps_route(int L, bool force_dense);  // force_dense: IMCOM_NOISEPS_ROUTE=dense (the caller reads the environment)
size_t noiseps_ws(int L, int nframe, int route);
int launch_noiseps_2d(imcom_ctx *ctx, const void *frames, bool in_f64, int nframe, int L, long fstride, long rstride, const double *window,
                      const double *norm_dev, bool bin8, int route, double *out);
int launch_noiseps_radial(imcom_ctx *ctx, const double *image, int nframe, int n, const int *rbin, int nidx, double *mean, double *err);
int launch_noiseps_accumulate(imcom_ctx *ctx, const double *ps2d, const double *mean, const double *err, int nlayers, long npix, int nrad, int bins,
                              int coverage_bin, double *ps2d_all, double *ps1d_all);

// pcg64.hip: draws of numpy's PCG64 stream by position, and the cosmic-ray mask made of them.  state / offset: (low, high) halves;
// jumps [PCG64_JUMPS][2][2]: the (low, high) halves of A_j and C_j, the affine map of 2^j steps for the stream's increment (device memory)
constexpr int PCG64_JUMPS = 128;
int launch_pcg64_uniform(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const unsigned long long offset[2], long count,
                         double *out);
int launch_pcg64_uniform_at(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const long *pos, long count, double *out);

// ziggurat.hip: numpy's normal draws of a PCG64 stream, one chunk of `tiles` tiles of P positions from stream position `start` (128 bits;
// start_rel: the same counted from the call's offset).  The chain enters the chunk at offset entry0 with base0 draws made; res[2] = {entry
// offset after the chunk, draws made by then}.  exit_t / count_t [tiles][ZIG_ENTRIES], entry_t / base_t [tiles]: the tile tables.
// info [4] (device, zeroed by the caller): outputs consumed by `count` draws, slow attempts, tail draws, flags (1 undecided, 2 tail list full).
size_t zig_lds_bytes(int P, int levels);
int launch_zig_chunk(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const unsigned long long start[2],
                     unsigned long long start_rel, int P, long tiles, int entry0, long base0, double guard, unsigned char *exit_t, unsigned short *count_t,
                     unsigned char *entry_t, long *base_t, long *res, long count, double *out, long *tail_idx, unsigned long long *tail_raw, long tail_cap,
                     unsigned long long *info);
// noise1f.hip: the transform of the 1/f noise layer.  noise1f_split: len = N1 N2 for the four-step transform, false if len is no power of
// two in 2^10 .. 2^20.  launch_noise1f_group: channels ch0 .. ch0 + nchg - 1 of g [2 nch][len] into blk [nch][len / 2] (Re DFT / sqrt 2), S
// [nchg][len] complex scratch, tw1 [N1] / tw2 [N2] the stage tables of the line plans
// (noise1f_tables).  launch_noise1f_place: the channel sums (sum
// [nch]), blk minus its channel mean in place, and the float32 frame without its border.
constexpr int NOISE1F_GROUP = 8;  // channels that share one pass (and the scratch S: 128 MB at len = 2^20)
bool noise1f_split(long len, int *N1, int *N2);
int noise1f_tables(imcom_ctx *ctx, long len, double2 *tw1, double2 *tw2);
int launch_noise1f_group(imcom_ctx *ctx, const double *g, const double *amp, long len, int ch0, int nchg, const double2 *tw1, const double2 *tw2, double2 *S,
                         double *blk);
int launch_noise1f_place(imcom_ctx *ctx, double *blk, double *sum, long len, int nch, int w, int border, float *frame);
int launch_cr_mask(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, unsigned long long base, int nside, int pad, double pcut,
                   const float *labnoise, double threshold, unsigned char *mask, unsigned long long *ngood);

// objmask.hip: exact order statistics, threshold / clipping flags, constrained propagation, box dilation and application of a mask
constexpr int SELECT_BINS = 2048, SELECT_STATE = 8;  // histogram bins of a pass (two histograms); words of the selection state
constexpr int MASK_DILATE_TX = 48, MASK_DILATE_TY = 32, MASK_DILATE_MAX_R = 8;  // output pixels of a dilation workgroup; largest radius
constexpr int MASK_PROPAGATE_T = 62;                                            // side of a propagation tile
int launch_select_kth(imcom_ctx *ctx, const void *vals, bool f64, const unsigned char *flags, long n, bool use_abs, double c, long k, unsigned long long *state,
                      unsigned long long *hist, void *res, long *info);
int launch_mask_threshold(imcom_ctx *ctx, const void *img, bool f64, long n, double bkg, double t1, double t2, bool finite_only, unsigned char *m1,
                          unsigned char *m2);
int launch_mask_clip(imcom_ctx *ctx, const void *img, bool f64, long n, const unsigned char *keep_in, double bkg, double t, unsigned char *keep_out,
                     unsigned long long *count);
int launch_mask_apply(imcom_ctx *ctx, const void *in, int dtype, const unsigned char *mask, long n, void *out);
int launch_mask_dilate(imcom_ctx *ctx, const unsigned char *in, int H, int W, int r, unsigned char *out);
int launch_mask_propagate(imcom_ctx *ctx, const unsigned char *grow, int H, int W, unsigned char *out, unsigned char *tmp, unsigned int *changed, long *sweeps);

// quantiles.hip: the counting passes of the streaming exact select and the coded-map histogram.  QtDev: the accumulator's device state
// (all 64-bit words) -- per segment the elements and the NaNs the running pass has seen and the number of its live groups, `bad` one word
// (segment ids out of range, star positions not served), the ascending prefixes of segment s's groups at gprefix[s R ..], the group's
// counters at hist[(s R + g) QT_BINS ..].
constexpr int QT_BINS = 2048, QT_TILE = 8, QT_THREADS = 512;  // counters of a group; groups whose counters share a workgroup's LDS; its threads
struct QtDev {
    unsigned long long *tot, *nan, *ng, *bad, *gprefix, *hist;
    int S, R;
};
int launch_quant_dense(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, int ng, const void *p, long rows, long cols, long pitch, int shift, int nbits);
int launch_quant_ids(imcom_ctx *ctx, const QtDev &d, bool f64, const void *p, const void *ids, bool ids_i32, long n, int shift, int nbits);
int launch_quant_rings(imcom_ctx *ctx, const QtDev &d, bool f64, const void *frame, int n, long pitch, const double *x, const double *y, int nstar, int rpix, int shift,
                       int nbits);
int launch_quant_constant(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, double value, unsigned long long count, int shift, int nbits);
int launch_codehist(imcom_ctx *ctx, const unsigned short *codes, long rows, long cols, long pitch, const unsigned char *table, int nbins, unsigned long long *counts);

// i24.hip: the I24 layer codec for a batch of L layers of ny x nx pixels (n = ny nx, tiles = i24_tiles(n) of I24_TILE pixels, i24_core.h).
// pars [L] device records.  launch_i24_quantise: codes [L][n], counts [L][tiles] -> the exclusive prefix sums of the tiles' overflow hits,
// totals [L].  launch_i24_pack: codes -> I24A int32 / I24B bytes, layer l at out + l out_stride (bytes).  launch_i24_overflow: the table
// entries of layer l at layer_off[l] .. layer_off[l + 1] (device, [L + 1]) of oy / ox / ov, none at or beyond cap.  launch_i24_decode:
// in -> codes (SOFTBIAS undone), sums [L][tiles] and totals [L] scratch of the prefix sum, out [L][n] float32.  launch_i24_patch: the
// overflow entries into out; *status becomes non-zero if a position lies outside the image (it is not stored).
struct I24Par;
int launch_i24_quantise(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, int *codes, uint32_t *counts,
                        uint32_t *totals);
int launch_i24_pack(imcom_ctx *ctx, const int *codes, int L, long n, const I24Par *pars, int scheme, unsigned char *out, long out_stride);
int launch_i24_overflow(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, const uint32_t *bases,
                        const uint32_t *totals, const long *layer_off, long cap, int *oy, int *ox, float *ov);
int launch_i24_decode(imcom_ctx *ctx, const unsigned char *in, long in_stride, int scheme, int L, long n, const I24Par *pars, bool any_diff, int *codes, uint32_t *sums,
                      uint32_t *totals, float *out);
int launch_i24_patch(imcom_ctx *ctx, float *out, int L, int ny, int nx, const long *layer_off, long max_count, const int *oy, const int *ox, const float *ov,
                     unsigned int *status);

}  // namespace imcom
