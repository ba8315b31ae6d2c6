/*
 * imcom_hip.h -- C-ABI of libimcom_hip.so: the MI355X (gfx950) IMCOM postage-stamp path.
 *
 * This is the drop-in boundary for the ONE hot path of pyimcom (reference checkout paths below are
 * relative to src/pyimcom/): per-postage-stamp construction of the PSF-overlap system matrix A and
 * the target cross-correlation -B/2, the Cholesky / eigen solve T = (A + kappa I)^-1 (-B/2), the
 * leakage U/C, noise Sigma and kappa maps, and the coaddition epilogue.  Plain C, caller-allocated
 * buffers, no torch types.  Every entry point returns 0 (IMCOM_OK) or a negative imcom_status;
 * imcom_last_error() gives the message of the calling thread's last failure.
 *
 * Pointers are host or device pointers as selected by `memspace`: with IMCOM_MEM_HOST the library
 * stages through its own device workspace and the call is synchronous; with IMCOM_MEM_DEVICE the
 * work is enqueued on the context's stream (imcom_ctx_set_stream) and the call returns immediately
 * (small per-stamp arrays named "host" below are always host pointers).  One context per GPU and
 * caller thread; a context is not thread-safe.  There is NO CPU fallback anywhere in this library.
 *
 * All matrices are C-order (row-major) float64 unless stated.  N = selected input pixels of a
 * stamp, m = n2f*n2f output pixels, nv = number of kappa nodes, n_out = target PSFs (1 per call
 * here; the host mirror loops over n_out as the reference does, lakernel.py:165,291,349).
 */
#ifndef IMCOM_HIP_H
#define IMCOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMCOM_HIP_VERSION 100 /* 0.1.0 */
#define IMCOM_PAIR_SWAP (1 << 29)
#define IMCOM_PAIR_FLIP (1 << 30)

typedef enum {
    IMCOM_OK = 0,
    IMCOM_ERR_ARG = -1,         /* bad argument (null pointer, bad size, unaligned layout) */
    IMCOM_ERR_HIP = -2,         /* a HIP runtime call failed (no device, launch failure, ...) */
    IMCOM_ERR_NOMEM = -3,       /* device workspace allocation failed */
    IMCOM_ERR_UNSUPPORTED = -4, /* valid request this build cannot serve */
    IMCOM_ERR_NUMERIC = -5      /* non-finite input or a factorisation that cannot be repaired */
} imcom_status;

typedef enum { IMCOM_MEM_HOST = 0, IMCOM_MEM_DEVICE = 1 } imcom_memspace;

typedef struct imcom_ctx imcom_ctx;

/* ------------------------------------------------------------------ library / context --------- */
int imcom_version(void);
const char *imcom_last_error(void);
int imcom_device_count(int *count);
/* device: HIP device ordinal.  Creates the context's own stream; block->GPU farming uses one
 * context per GPU (one process per GPU), no inter-GPU traffic (docs/run_README.rst:81-100). */
int imcom_ctx_create(int device, imcom_ctx **ctx);
int imcom_ctx_destroy(imcom_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) for all subsequent work; NULL is the
 * legacy default stream (torch's default stream).  A fresh context runs on its own stream. */
int imcom_ctx_set_stream(imcom_ctx *ctx, void *hip_stream);
int imcom_ctx_sync(imcom_ctx *ctx);
/* Bytes of device workspace currently held by the context (grows on demand, never inside a call
 * whose sizes were seen before). */
int imcom_ctx_workspace_bytes(imcom_ctx *ctx, size_t *bytes);
/* Give the workspace back to the device (after draining the context's streams); the next call allocates what it needs.
 * For drivers that change kernel or batch size between blocks: the workspace otherwise keeps the size of the largest call. */
int imcom_ctx_workspace_release(imcom_ctx *ctx);
/* ONE OWNER for device memory.  By default a context allocates its workspace itself (hipMalloc, growing on demand).  After this
 * call it works in the caller's buffer `ptr` of `bytes` bytes (256-byte aligned; NULL, 0 = "none yet") and never allocates device
 * memory again: a call that needs more returns IMCOM_ERR_NOMEM without having queued anything, imcom_ctx_workspace_needed says how
 * much it asked for, and the caller -- who knows what else lives on the device -- provides it or plans smaller.  The buffer must
 * stay valid until the next imcom_ctx_set_workspace / imcom_ctx_destroy; imcom_ctx_workspace_release only forgets it.  The
 * reference's analogue is TEMPFILE, its "virtual memory" for A sub-blocks (psfutil.py:2056-2085): where they live is the user's call.
 * pyimcom_amd.Context takes the buffer from torch's allocator, so that torch is the only allocator on the device. */
int imcom_ctx_set_workspace(imcom_ctx *ctx, void *ptr, size_t bytes);
/* Workspace bytes the most recent call on this context asked for (whether or not it got them). */
int imcom_ctx_workspace_needed(imcom_ctx *ctx, size_t *bytes);
/* Elapsed device milliseconds spent in the named kernel family since the last reset, measured with
 * HIP events on the context's stream when profiling is enabled (bench.py's roofline leg).
 * family: "solve_gemm", "chol_gemm", "chol_diag", "build_A", "build_B", "finalize", "epilogue",
 *         "eigen", "lakernel1", ... ; launches receives the number of launches accumulated. */
int imcom_ctx_profile_enable(imcom_ctx *ctx, int on); /* on = 2: also per-launch scopes inside long stages ("symv4": the band reduction's pass over the trailing matrix) */
int imcom_ctx_profile_reset(imcom_ctx *ctx);
int imcom_ctx_profile_get(imcom_ctx *ctx, const char *family, double *ms, long *launches);
/* Diagnostic for the roofline: keeps the fp64 MFMA pipe of every SIMD busy -- and nothing else: no LDS, no memory, no
 * barriers -- for about `millis` ms and reports the rate reached [TFLOP/s]: the ceiling of this chip at the clock it holds under
 * matrix load, to set beside the guide's 78.6 TFLOP/s. */
int imcom_ctx_mfma_probe(imcom_ctx *ctx, double millis, double *tflops);
/* Diagnostic: the k loop of the tile engine as a plain batched product C[M][N] = A[M][K] (row-major) B[K][N] on pseudo-random
 * operands in workspace, `reps` launches; variant 0: the production 128 x 128 tiles (two 8-wave workgroups per CU); variants 2, 3, 4:
 * the same tiles on the engine's other operand layouts (both row-major; both k-major; A k-major, B row-major).  Any other variant is
 * IMCOM_ERR_ARG.  M % 256 = N % 128 = K % 16 = 0. */
int imcom_ctx_gemm_probe(imcom_ctx *ctx, int variant, int M, int N, int K, int batch, int reps, double *tflops);

/* ------------------------------------------------------------------ native-routine seam --------
 * Replaces furry_parakeet.pyimcom_croutines.* (imported at lakernel.py:41-47, psfutil.py:37-49),
 * whose in-tree specification is routine.py.  Outputs are written in place; off-grid points of the
 * scattered interpolators leave the output element untouched (routine.py:166-167, 231-232). */

/* routine.py:29-122 iD5512C_getw: w[i*10 .. i*10+9] = the 10 taps for fh[i] (fh = frac - 1/2). */
int imcom_d5512_getw(imcom_ctx *ctx, const double *fh, long n, double *w, int memspace);
/* routine.py:125-181 iD5512C (sym=0) / 184-253 iD5512C_sym (sym=1; nout must be a square, only the
 * upper triangle is interpolated and mirrored).  infunc[nlayer][ngy][ngx], fhatout[nlayer][nout]. */
int imcom_interp_d5512(imcom_ctx *ctx, const double *infunc, int nlayer, int ngy, int ngx,
                       const double *xpos, const double *ypos, long nout, double *fhatout, int sym,
                       int memspace);
/* routine.py:256-338 gridD5512C: infunc[ngy][ngx], xpos[npi][nxo], ypos[npi][nyo],
 * fhatout[npi][nyo*nxo]; off-grid rows/columns contribute zero weight (306-323). */
int imcom_grid_d5512(imcom_ctx *ctx, const double *infunc, int ngy, int ngx, const double *xpos,
                     const double *ypos, long npi, int nxo, int nyo, double *fhatout, int memspace);
/* routine.py:341-430 lakernel1: per-output-pixel geometric bisection on kappa.
 * lam[n], mPhalf[m][n] -> kappa[m], Sigma[m], UC[m], T[m][n] (T still to be multiplied by Q^T). */
int imcom_lakernel1(imcom_ctx *ctx, const double *lam, const double *mPhalf, long m, long n,
                    double C, double targetleak, double kCmin, double kCmax, int nbis,
                    double *kappa, double *Sigma, double *UC, double *T, double smax, int memspace);
/* routine.py:487-588 build_reduced_T_wrap (with lsolve_sps 433-484 inside).
 * Nflat[m*nv*nv], Dflat[m*nv], Eflat[m*nv*nv], kappa[nv] ascending -> out_*[m], out_w[m*nv]. */
int imcom_build_reduced_T(imcom_ctx *ctx, const double *Nflat, const double *Dflat,
                          const double *Eflat, const double *kappa, int nv, long m, double ucmin,
                          double smax, double *out_kappa, double *out_Sigma, double *out_UC,
                          double *out_w, int memspace);

/* ------------------------------------------------------------------ LA-kernel seam --------------
 * Replaces lakernel.CholKernel (lakernel.py:226-394) and lakernel.EigenKernel (141-223) behind the
 * OutStamp.LAKERNEL registry (coadd.py:839-844, 1091-1093), batched over independent stamps.
 *
 *   batch        number of stamps
 *   n[batch]     HOST array: input pixels per stamp (ragged batches allowed; n[s] == 0 gives the
 *                lakernel.py:110-119 outputs UC=1, Sigma=0, kappa=1 and no T)
 *   ldn          row stride (elements) and per-stamp extent of A: A[s] is at A + s*ldn*ldn, row i at
 *                + i*ldn; likewise B rows / T rows are ldn long.  ldn >= max n.
 *   m            output pixels per stamp
 *   A            [batch][ldn][ldn] system matrices (only the leading n[s] x n[s] part is read;
 *                never modified: coadd.py keeps using outst.sysmata when save_abc is set)
 *   mBhalf       [batch][m][ldn]  -B/2 in the reference layout (lakernel.py:287)
 *   C            [batch] HOST: target normalisation (psfutil.py:1290 outovlc)
 *   kappaC[nv]   HOST: kappa/C nodes, ascending (config KAPPAC); nv==1 -> single-kappa path
 *   T            [batch][m][ldn] float32 out (reference dtype, lakernel.py:122)
 *   UC,Sigma,kappa [batch][m] float32 out
 *   info[batch]  HOST out: 0 ok; >0 = the Cholesky repair of lakernel.py:262-279 was applied
 *                (value = node index + 1 of the first repaired factorisation)
 */
int imcom_solve_chol(imcom_ctx *ctx, int batch, const int *n, int ldn, int m, const double *A,
                     const double *mBhalf, const double *C, const double *kappaC, int nv,
                     double ucmin, double smax, float *T, float *UC, float *Sigma, float *kappa,
                     int *info, int memspace);
/* lakernel.CholKernel (lakernel.py:226-394) for SEVERAL OutStamps per call -- e.g. the four OutStamps that share the PSF overlap
 * of a 2 x 2 group (coadd.py:1091-1093 calls the kernel of one OutStamp at a time) -- each with its own HOST arrays as the
 * reference holds them: A[s] = outst.sysmata [n[s]][n[s]], mBhalf[s] = outst.mhalfb[j_out] [m][n[s]], T[s] [m][n[s]] float32,
 * UC[s] / Sigma[s] / kappa[s] [m] float32; C[nst], info[nst] as in imcom_solve_chol.  One batched factorisation and solve for
 * all stamps; -B/2 crosses PCIe behind the factorisation.  n[s] == 0 gives the lakernel.py:110-119 outputs and no T. */
int imcom_solve_chol_stamps(imcom_ctx *ctx, int nst, const int *n, int m, const double *const *A,
                            const double *const *mBhalf, const double *C, const double *kappaC, int nv, double ucmin,
                            double smax, float *const *T, float *const *UC, float *const *Sigma, float *const *kappa,
                            int *info);
/* Same contract, eigendecomposition path; nv==1: lakernel.py:154-172, nv>1: 174-223 with nbis
 * bisections (reference default 13) and the kappa *= C quirk of line 222.
 * info[s]: 0 = A + kappaC[0] C I is positive definite (the PSF-overlap matrices of this problem): solved in the band basis
 * (DESIGN.md "Eigen path"); 1 = it is NOT -- A has an eigenvalue at or below -kappaC[0] C, every pivot of the reduced matrix
 * is checked -- and the stamp was solved through the eigendecomposition itself with the reference's own formulas, which
 * divide by lam_i + kappa whatever its sign (numpy.linalg.eigh at lakernel.py:162, 201; routine.lakernel1): the kernel a
 * user falls back to when Cholesky fails serves any symmetric A.  Results are valid either way; never an error. */
int imcom_solve_eigen(imcom_ctx *ctx, int batch, const int *n, int ldn, int m, const double *A,
                      const double *mBhalf, const double *C, const double *kappaC, int nv,
                      double ucmin, double smax, int nbis, float *T, float *UC, float *Sigma,
                      float *kappa, int *info, int memspace);
/* Bytes of device workspace imcom_solve_eigen_resident takes for `batch` stamps of these leading dimensions (a planner adds
 * them to its own buffers: pyimcom_amd.blockrun.stamp_bytes).  Pure arithmetic: no context, no device call. */
int imcom_solve_eigen_workspace(int batch, int ldn, int ldm, int m, size_t *bytes);
/* The same for imcom_solve_chol_resident / _begin / _redo (nv kappa nodes; the repair path's scratch included). */
int imcom_solve_chol_workspace(int batch, int ldn, int m, int ldm, int nv, size_t *bytes);
/* Householder reduction of symmetric matrices to band form, the basis the Eigen kernel's kappa search works in
 * (numpy.linalg.eigh at lakernel.py:162, 201 is not needed for it: DESIGN.md "Eigen path"): A = Q B Q^T, B[i][j] = 0 for
 * |i - j| > 4, Q = H_0 H_1 ... with H_r = I - tau_r v_r v_r^T, v_r zero above its pivot row r + 4 (v_r[r+4] = 1).
 *   A     [batch][ldn][ldn] symmetric, leading n[s] x n[s] used; ldn a multiple of 128, at most 4864 (the N x 4 panel lives in LDS)
 *   band  [batch][5][ldn] out: band[t][i] = B[i+t][i];  V [batch][ldn][ldn] out: row r = v_r;  tau [batch][ldn] out */
int imcom_band_reduce(imcom_ctx *ctx, int batch, const int *n_host, int ldn, const double *A, double *band, double *V,
                      double *tau, int memspace);
/* The same kernel on the resident layouts of imcom_build_A / imcom_build_B (DEVICE pointers): A [batch][ldn][ldn], Bt = -B/2
 * input-pixel-major [batch][ldn][ldm] (zero padded), output Tt [batch][ldn][ldm] float32; ldn, ldm multiples of 128.
 * EigenKernel._call_single_kappa / _call_multi_kappa (lakernel.py:154-223) without the transposes of the reference layout. */
int imcom_solve_eigen_resident(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, const double *A,
                               const double *Bt, const double *C_host, const double *kappaC_host, int nv, double ucmin,
                               double smax, int nbis, float *Tt, float *UC, float *Sigma, float *kappa, int *info_host);

/* ---- secondary LA kernels: lakernel.IterKernel 533-744, lakernel.EmpirKernel 747-805 ----------------------
 * Geometry (all in output-pixel units, as the reference computes them at lakernel.py:617-622 / 757-761):
 *   out_yx  [batch][2][m]  outst.yx_val: y then x of every output pixel (row-major over the n2f x n2f stamp)
 *   in_y,in_x [batch][ldn] outst.iny_val / inx_val
 *   rho_acc = (cfg.instamp_pad / arcsec) / (cfg.dtheta * 3600): acceptance radius
 * n, C, kappaC are HOST arrays as for imcom_solve_chol; the other pointers follow `memspace`.
 *
 * imcom_solve_iter: per output pixel, conjugate gradients (lakernel.py:397-442: x0 = 0, stop at |r| < rtol |b| or
 * after maxiter steps) on the sub-system of the input pixels with hypot(dy, dx) < rho_acc; T is float32 and zero
 * outside the disc.  nv == 1: lines 588-654; nv > 1: 656-744 (node solutions combined by build_reduced_T_wrap).
 * exact_UC selects E = T A T^T (reference default for nv > 1) against the approximation D - kappa N (default for
 * nv == 1).  At most 4096 input pixels per acceptance disc (IMCOM_ERR_ARG beyond). */
int imcom_solve_iter(imcom_ctx *ctx, int batch, const int *n, int ldn, int m, const double *A,
                     const double *mBhalf, const double *C, const double *kappaC, int nv, double ucmin,
                     double smax, const double *out_yx, const double *in_y, const double *in_x,
                     double rho_acc, double rtol, int maxiter, int exact_UC, float *T, float *UC,
                     float *Sigma, float *kappa, int memspace);
/* What the last imcom_solve_iter call on this context did at its LAST kappa node (the reference has no counterpart: its
 * conjugate_gradient, lakernel.py:397-442, returns x only; a parity test of recurrences that stop at maxiter needs the step
 * counts, and the bench its roofline).  stats[8] (host): [0] 4 x 4 patches solved by the blocked solver, [1] sum over the
 * patches of (union size rounded up to 16)^2 x steps the patch ran (x 2 x 16 = its flops, x 8 = the bytes of sub-matrix it
 * streamed by the full-storage kernel), [2] sum of steps, [3] sum of (union size)^2, [4] largest union of a patch, [5] 1 = blocked
 * solver, 0 = the per-pixel kernel (a union above 1024), [6] bytes of sub-matrix the patches streamed over their steps, [7] 1 = the
 * half-storage kernel (unions up to 864: only the tiles on and below the diagonal are stored and read).  steps (host, optional): CG steps used per output pixel
 * [batch][m], nsteps = batch * m of that call. */
int imcom_solve_iter_stats(imcom_ctx *ctx, double *stats, int *steps, long nsteps);
/* imcom_solve_empir: T_ai = max(rho_acc - dist_ai, 0) / sum_i max(rho_acc - dist_ai, 0) (a pixel with no input
 * pixel in range gets NaN, as in the reference); kappa = kappaC0 * C, Sigma = sum T^2, UC = 1 + (T A T^T - 2 D)/C.
 * no_qlt_ctrl != 0 (cfg.no_qlt_ctrl, coadd.py:856-858): only T is produced, A / mBhalf / C may be NULL and the
 * maps are zero (lakernel.py:774-777). */
int imcom_solve_empir(imcom_ctx *ctx, int batch, const int *n, int ldn, int m, const double *A,
                      const double *mBhalf, const double *C, double kappaC0, const double *out_yx,
                      const double *in_y, const double *in_x, double rho_acc, int no_qlt_ctrl, float *T,
                      float *UC, float *Sigma, float *kappa, int memspace);
/* Batched symmetric eigendecomposition used by the eigen path and by the Cholesky repair
 * (replaces numpy.linalg.eigh at lakernel.py:162,201,266): lam ascending [batch][ldn],
 * Q[batch][ldn][ldn] with eigenvectors in columns.  A is not modified. */
int imcom_eigh(imcom_ctx *ctx, int batch, const int *n, int ldn, const double *A, double *lam,
               double *Q, int memspace);

/* ------------------------------------------------------------------ stamp / matrix seam ---------
 * Device-resident replacement of PSFOvl._call_ii_self/_call_ii_cross (psfutil.py:1597-1732,
 * 1401-1495) + OutStamp A assembly (coadd.py:1027-1068), PSFOvl._call_io_cross (1497-1595) +
 * B assembly (coadd.py:1075-1082), and OutStamp._perform_coaddition (coadd.py:1294-1363).
 * These take DEVICE pointers only (except arrays marked HOST). */

/* Geometry shared by the table interpolations (PSFGrp.setup / PSFOvl.setup class attributes,
 * psfutil.py:568-613, 1065-1089, carried explicitly instead of process-global state). */
typedef struct {
    int nsamp;           /* PSFOvl.nsamp.  Tables handed to the builders carry the 6-pixel zero border
                            of np.pad(..., 6) (psfutil.py:1471-1473, 1580, 1696): [nsamp+12][nsamp+12] */
    double nc;           /* PSFOvl.nc, table centre */
    double dscale;       /* PSFGrp.dscale: output pixels per table sample */
    double flat_penalty; /* PSFOvl.flat_penalty */
} imcom_table_geom;

/* ---- pixel partition: the binning loop of InImage.partition_pixels coadd.py:329-358 (device pointers only) ----
 * The host visits the relevant sparse-grid cells in order and evaluates the WCS (coadd.py:335-336); what it hands
 * over, in visiting order: out_x, out_y [npix] f64 (position in output-block pixels), in_x, in_y [npix] u16 (index in
 * the input image), mask [npix] u8 (0 = masked; NULL = none), use_instamps [nst][nst] u8 (blk.use_instamps, nst =
 * n1P + 2).  A pixel is kept when pix_lower < x, y < pix_upper, unmasked, and its stamp (j_st, i_st) =
 * floor((pos - pix_lower) / n2) is in use; kept pixels are appended to their stamp in visiting order:
 * y_idx, x_idx u16 and y_val, x_val f64 [nst][nst][npixmax], pix_count u32 [nst][nst].
 * IMCOM_ERR_ARG if a stamp would receive more than npixmax pixels (the reference's arrays overflow there). */
int imcom_partition_pixels(imcom_ctx *ctx, long npix, const double *out_x, const double *out_y,
                           const unsigned short *in_x, const unsigned short *in_y, const unsigned char *mask,
                           const unsigned char *use_instamps, int nst, int n2, double pix_lower,
                           double pix_upper, int npixmax, unsigned short *y_idx, unsigned short *x_idx,
                           double *y_val, double *x_val, unsigned int *pix_count);

/* ---- input-pixel selection: OutStamp._process_input_stamps coadd.py:886-977 + InStamp.make_selection 716-749 ----
 * The block's InStamps lie back to back in a pool:
 *   pool_x, pool_y [npool] f64 (InStamp.x_val / y_val), pool_data [n_inframe][npool] f32 (InStamp.data),
 *   pool_expo [npool] i32 (exposure index of each pixel, from InStamp.pix_cumsum),
 *   inst_off [n_inst+1]: InStamp i owns pool[inst_off[i] : inst_off[i+1]].
 * Per output stamp s and neighbour idx = 0..8 (row-major over dj, di = -1..1, coadd.py:878):
 *   inst_id [batch][9] InStamp index or -1; pivot_x / pivot_y [batch][9] (NaN = None, lines 918-919);
 *   radius = rpix_search (line 912; NaN = select everything).
 * A pixel is kept when (x - px)^2 + (y - py)^2 < radius^2 (terms of missing pivot coordinates dropped), in pool
 * order.  Outputs x, y [batch][ldn], indata [batch][n_inframe][ldn], expo [batch][ldn] (zero padded) and
 * cumsum [batch][10] = inpix_cumsum; n[s] = cumsum[s][9].  IMCOM_ERR_ARG if a stamp selects more than ldn. */
int imcom_select_pixels(imcom_ctx *ctx, int batch, const double *pool_x, const double *pool_y,
                        const float *pool_data, long npool, int n_inframe, const int *pool_expo,
                        const long *inst_off, int n_inst, const int *inst_id, const double *pivot_x,
                        const double *pivot_y, double radius, int ldn, double *x, double *y, float *indata,
                        int *expo, int *cumsum, int memspace);

/* A[s][i][j] for i,j < n[s] (exactly symmetric: the element with i before j is interpolated and
 * mirrored, as the reference's sub-block assembly does, coadd.py:1038-1068), with the
 * padding rows/cols n[s] <= i < ldn set to the identity so the factorisation kernels can run on
 * whole tiles.
 *   x,y          [batch][ldn] input pixel positions in output-pixel units (coadd.py:969-972)
 *   psf          [batch][ldn] int32: stamp-local PSF index of each pixel, < npsf_max
 *   tables       [ntab][nsamp+12][nsamp+12] zero-bordered overlap tables (PSFOvl.ovl_arr entries)
 *   pair_tab     [batch][npsf_max][npsf_max] int32 code of the ordered PSF pair (p_i,p_j), i before j:
 *                bits 0..27 table index; bit 30 (IMCOM_PAIR_FLIP) = table flipped in both axes (the
 *                np.flip of psfutil.py:1658-1665); bit 29 (IMCOM_PAIR_SWAP) = the reference evaluated
 *                this block from the other stamp's side and transposed it (psfutil.py:1990-1996), i.e.
 *                interpolate at r_j - r_i; negative = no table (value 0 + penalty)
 *   pair_pen     [batch][npsf_max][npsf_max] constant added to every element of the pair's block:
 *                -flat_penalty/n_in (+flat_penalty for the same exposure), psfutil.py:1482-1486,
 *                1705-1708
 */
int imcom_build_A(imcom_ctx *ctx, int batch, const int *n_host, int ldn, const double *x,
                  const double *y, const int *psf, const double *tables, int ntab,
                  const imcom_table_geom *geom, const int *pair_tab, const double *pair_pen,
                  int npsf_max, double *A);
/* Bt[s][i][a] = -B/2 transposed (input-pixel-major, the native layout of gridD5512C's output,
 * routine.py:273) for i < n[s], a < m = n2f*n2f; rows i >= n[s] and columns a >= m up to ldm are
 * zero.  Output pixel a = iy*n2f + ix sits at (out_x0[s] + ix, out_y0[s] + iy) (coadd.py:879-882).
 *   io_tab       [batch][npsf_max] int32: input-output overlap table of each stamp-local PSF
 */
int imcom_build_B(imcom_ctx *ctx, int batch, const int *n_host, int ldn, const double *x,
                  const double *y, const int *psf, const double *tables, int ntab,
                  const imcom_table_geom *geom, const int *io_tab, int npsf_max,
                  const double *out_x0, const double *out_y0, int n2f, int ldm, double *Bt);
/* Resident single/multi-kappa Cholesky solve on the layouts produced by imcom_build_A/_B:
 * A[batch][ldn][ldn] (padding = identity), Bt[batch][ldn][ldm].  Outputs: Tt[batch][ldn][ldm]
 * float32 (input-pixel-major), UC/Sigma/kappa [batch][m] float32.  Needs ldn, ldm multiples of 128. */
int imcom_solve_chol_resident(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm,
                              const double *A, const double *Bt, const double *C_host,
                              const double *kappaC_host, int nv, double ucmin, double smax,
                              float *Tt, float *UC, float *Sigma, float *kappa, int *info_host);
/* imcom_solve_chol_resident in two halves, for a caller with host work to do while the device factors and solves
 * (the reference's loop is synchronous, lakernel.py:84-138; a block driver prepares its next pass in between).
 * _begin queues the whole first attempt and returns.  _end waits for it: every A + kappa I positive definite (the
 * normal case) -> info = 0, IMCOM_OK, outputs final; otherwise _end returns 1 with info[s] != 0 for the stamps whose
 * factorisation failed (the other stamps' outputs are final) and the caller runs imcom_solve_chol_resident_redo on those
 * (one kappa node) or imcom_solve_chol_resident on the same arguments (the eigh-shift repair of lakernel.py:262-279).  Work queued on the
 * context between the two calls runs behind the solve; a begin whose _end never came is waited for and forgotten by the next begin. */
int imcom_solve_chol_resident_begin(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm,
                                    const double *A, const double *Bt, const double *C_host,
                                    const double *kappaC_host, int nv, double ucmin, double smax,
                                    float *Tt, float *UC, float *Sigma, float *kappa);
int imcom_solve_chol_resident_end(imcom_ctx *ctx, int batch, int *info_host);
/* CholKernel._call_single_kappa (lakernel.py:281-323) for SOME stamps of a resident batch: redo_host[s] = 0 leaves stamp s and
 * its outputs untouched, 1 solves it, 2 solves it knowing that the factorisation of A + kappa I fails (what _end reported), i.e.
 * straight to _cholesky_wrapper's repair (lakernel.py:262-279: AA_ii += |w[0]| + 1e-16 with w[0] the smallest eigenvalue of A),
 * 3 the same on the caller's EXPECTATION (the stamps before it failed; a stamp whose A + kappa I is positive definite after all is
 * recognised and solved without the repair).  nv must be 1.  info as imcom_solve_chol_resident, written for the stamps that were solved. */
int imcom_solve_chol_resident_redo(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm,
                                   const double *A, const double *Bt, const double *C_host,
                                   const double *kappaC_host, int nv, double ucmin, double smax,
                                   float *Tt, float *UC, float *Sigma, float *kappa, const int *redo_host, int *info_host);
/* _cholesky_wrapper's repair (lakernel.py:262-279) needs w[0], the smallest eigenvalue of a failed stamp's A; the library finds it by
 * inverse subspace iteration, which starts from a shift sigma with A + sigma I positive definite.  A driver that
 * has just repaired neighbouring stamps knows where w[0] lies: imcom_ctx_set_repair_hint(ctx, h) with h ~ max |w[0]| of those stamps
 * makes the following Cholesky calls on this context start at h (1 + 5 %) -- one factorisation inside the iteration instead of two.  The
 * hint changes the iteration's path, not what it converges to (w[0] to 1e-11 either way; a hint that is too small for a stamp costs that
 * stamp one failed factorisation).  0 clears it.  imcom_ctx_last_repair: how many stamps the last Cholesky call repaired and the range
 * of their w[0] (count = 0: none, the range is then 0). */
int imcom_ctx_set_repair_hint(imcom_ctx *ctx, double lmin_abs);
/* The same knowledge for the host-array entries (imcom_solve_chol, imcom_solve_chol_stamps; one kappa node): expect != 0 makes the
 * following calls on this context skip the factorisation of A + kappa I that a driver has just seen fail on the neighbouring stamps and
 * go straight to the repair (lakernel.py:262-279) -- the resident path's redo code 2.  A stamp whose A + kappa I is positive definite
 * after all is recognised by the smallest-eigenvalue iteration and solved without the repair (same outputs, one wasted iteration).
 * 0 clears it. */
int imcom_ctx_set_repair_expect(imcom_ctx *ctx, int expect);
int imcom_ctx_last_repair(imcom_ctx *ctx, int *count, double *w0_min, double *w0_max);
/* coadd.py:1320-1354: fade taper of T (trapezoid, 1222-1292), per-exposure weight sums, Neff and
 * outimage = T . indata.
 *   Tt           [batch][ldn][ldm] float32 (tapered in place when fade > 0)
 *   indata       [batch][n_inframe][ldn] float32 input pixel values (coadd.py:975)
 *   expo         [batch][ldn] int32 exposure (input image) index of each pixel, < n_expo
 *   outimage     [batch][n_inframe][m] float32
 *   Tsum_stamp   [batch][n_expo] float64; Tsum_inpix, Neff [batch][m] float64 (numpy's result dtype)
 * ldm must be a multiple of 128 (the layout imcom_build_B and the resident solves leave) and ldn >= every n[s]; n_expo <= 64.  Rows
 * i >= n[s] and columns a >= m of Tt, indata[..][i >= n[s]] and expo[i >= n[s]] enter no output (with fade > 0 the columns m .. m + 2 of Tt
 * may be overwritten).
 */
int imcom_coadd_epilogue(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm,
                         int n2f, int fade, int n2, float *Tt, const float *indata, int n_inframe,
                         const int *expo, int n_expo, float *outimage, double *Tsum_stamp,
                         double *Tsum_inpix, double *Neff);
/* imcom_solve_chol_resident and imcom_coadd_epilogue in ONE call, for fade == 0 (with fade > 0 the map tapers of
 * coadd.py:1118-1122 come in between: use the three calls): CholKernel (lakernel.py:281-394) on the device layouts, then
 * OutStamp._perform_coaddition (coadd.py:1294-1363) for the same stamps.  With one kappa node the coaddition's sums -- per
 * exposure sum_j T[a][j] and per input frame sum_j T[a][j] indata[j] -- are taken from the tiles of T while the backward
 * launches of the solve still hold them, so T (20 MB per stamp) is not read again; with several nodes the stand-alone
 * epilogue runs inside the call.  Arguments as in the two entries; all pointers DEVICE except n_host / C / kappaC / info. */
int imcom_solve_chol_resident_coadd(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm,
                                    const double *A, const double *Bt, const double *C, const double *kappaC, int nv,
                                    double ucmin, double smax, float *Tt, float *UC, float *Sigma, float *kappa,
                                    int *info, int n2f, int fade, int n2, const float *indata, int n_inframe,
                                    const int *expo, int n_expo, float *outimage, double *Tsum_stamp,
                                    double *Tsum_inpix, double *Neff);
/* OutStamp.trapezoid (coadd.py:1222-1292) on [batch][n2f][n2f] float32 maps (kappa, Sigma, UC). */
int imcom_trapezoid_f32(imcom_ctx *ctx, float *maps, long nmaps, int n2f, int fade);
/* OutStamp._build_system_matrices, coadd.py:1104-1107: after the "Iterative" kernel (whose U/C and Sigma can come
 * out negative) the reference sets UC = np.maximum(UC, 1e-32), Sigma = np.maximum(Sigma, 1e-32), before the map
 * taper.  maps[i] = maps[i] < lo ? lo : maps[i] on `count` device float32 values; NaN stays NaN (np.maximum). */
int imcom_clamp_min_f32(imcom_ctx *ctx, float *maps, long count, float lo);

/* Block._output_stamp_wrapper map updates (coadd.py:1975-1993), on the device: for every stamp s of the batch,
 * dst[layer][(jst-1)*n2 + r][(ist-1)*n2 + c] += src[s][layer][r][c], r,c < n2f = n2 + 2*fade.  dst is one of the
 * block's float32 maps [nlayer][nside_pf][nside_pf] (out_map with nlayer = n_inframe; UC/Sigma/kappa/Tsum/Neff
 * with nlayer = 1); src is float32 or float64 (src_is_f64).  jst/ist are HOST arrays of 1-based OutStamp
 * indices.  Overlapping neighbours are added in four index-parity passes, so the result is deterministic. */
int imcom_block_accumulate(imcom_ctx *ctx, int batch, const int *jst_host, const int *ist_host, int n2, int fade,
                           int nlayer, const void *src, int src_is_f64, float *dst, int nside_pf);
/* The same map updates for OVERLAPPING stamps (fade > 0) without a dependence on the visiting order.  A block pixel belongs
 * to at most four stamps, one of each index parity ((jst & 1) << 1 | (ist & 1)).  imcom_block_place STORES every stamp's
 * tile, in the dtype it arrives in, into the layer of its parity: layers [4][nlayer][nside_pf][nside_pf] float32 or
 * float64 (src_is_f64), zero before the first call.  imcom_block_combine then forms dst[layer][row][col] by adding the
 * layers of a pixel in the order in which the reference's loop meets their stamps -- order = 1: coadd.py:2056-2059, cells of
 * 2 x 2 stamps from (j_st_min, i_st_min) on (coadd.py:1808-1838), row by row of cells, inside a cell dj outer, di inner;
 * order = 0: plain rows, j_st outer, i_st inner -- every addition rounded as numpy's `f32_map[window] += tile` (float32 +
 * float32 -> float32; float32 + float64 in double, rounded once): the result carries the reference's own rounding whatever
 * batches, passes or processes the stamps were dealt to (pyimcom_amd.farm shares a block's passes between GPUs).
 * dst: [nlayer][nside_pf][nside_pf] float32, nside_pf = n1P * n2 + 2 * fade. */
int imcom_block_place(imcom_ctx *ctx, int batch, const int *jst_host, const int *ist_host, int n2, int fade, int nlayer,
                      const void *src, int src_is_f64, void *layers, int nside_pf);
int imcom_block_combine(imcom_ctx *ctx, int n1P, int n2, int fade, long nlayer, const void *layers, int src_is_f64,
                        float *dst, int nside_pf, int order, int j_st_min, int i_st_min);
/* Block.build_output_file boundary recovery (coadd.py:2163-2181): OutStamp.trapezoid(maps, fade,
 * recover_mode=True, pad_widths=(b,t,l,r)) on float32 maps [nmaps][ny][nx]. */
int imcom_trapezoid_recover_f32(imcom_ctx *ctx, float *maps, long nmaps, int ny, int nx, int fade, int pad_b,
                                int pad_t, int pad_l, int pad_r);
/* Block.compress_map coadd.py:2087-2138 (device pointers): out[i] = clip(floor(coef * log10(clip(map[i], 1e-32, inf))
 * + 0.5), a_min, a_max) in float32 arithmetic, as int16 (is_unsigned = 0) or uint16 (1).  The reference's
 * coefficients (coadd.py:2249-2303): U/C -5000 uint16, Sigma -10000 int16, kappa -5000 uint16, Tsum 200000 int16,
 * Neff 50000 uint16. */
int imcom_compress_map_f32(imcom_ctx *ctx, const float *map, long count, int coef, int is_unsigned, void *out);

/* ---- PSF images -> sample grid, target PSFs --------------------------------------------------------------
 * imcom_sample_psf: PSFGrp._sample_psf psfutil.py:709-795 followed by the circular cut-out / normalisation of
 * PSFGrp.__init__ 650-656.  psf [n_psf][ny][nx]; yxco [n_psf][2][nsamp*nsamp] = y then x offsets of the sampling
 * positions from the image centre in oversampled native pixels (the host computes them through the WCS,
 * psfutil.py:751-771), or NULL for the unrotated grid PSFGrp.yxo (the target-PSF path, evaluated with gridD5512C
 * as the reference does at 786-793).  psf_arr [n_psf][nsamp][nsamp] out; samples off the image stay zero. */
int imcom_sample_psf(imcom_ctx *ctx, int n_psf, const double *psf, int ny, int nx, const double *yxco,
                     int nsamp, int psf_circ, int psf_norm, double *psf_arr, int memspace);
/* The sampling positions yxco of imcom_sample_psf from a coarse lattice: the reference evaluates outpix2world2inpix at all
 * nsamp^2 positions of a PSF group and exposure (psfutil.py:751-771: 146 689 WCS evaluations, the host half of the Block seam);
 * over the ~5" they span that map is smooth, so a caller may evaluate it on an L x L lattice of Chebyshev-Lobatto nodes
 * u_a = u_mid + u_half cos(pi a / (L - 1)) of the sample coordinate and hand over
 *   lattice [count][2][L][L]  the offsets (y plane then x plane, as yxco) at lattice point (node a along y, node b along x)
 *   W       [nsamp][L] (HOST) W[i][a] = Lagrange basis polynomial a of the nodes at sample coordinate i
 * yxco[c][k][iy][ix] = sum_a sum_b W[iy][a] W[ix][b] lattice[c][k][a][b] -- exact for maps of degree < L per axis (an affine WCS,
 * SIP distortion up to order L - 1), 2 <= L <= 33.  lattice / yxco follow `memspace`. */
int imcom_lattice_positions(imcom_ctx *ctx, int count, int L, const double *W, const double *lattice, int nsamp,
                            double *yxco, int memspace);
/* The sampling positions yxco of imcom_sample_psf under PSFSPLIT (PSFGrp._sample_psf, psfutil.py:739-753): the reference evaluates
 * outpix2world2inpix at the group's computation point +- oversamp output pixels along x and y only,
 *   cardinal [count][4][2] = flip(outpix2world2inpix(p0 + [[1,0],[0,1],[-1,0],[0,-1]] * oversamp), axis=-1) / 2 * dscale   (y, x),
 * and takes the map as affine over the PSF window: yxco[c][k][iy][ix] = (c0 - c2)[k] * yxo[1][iy][ix] + (c1 - c3)[k] * yxo[0][iy][ix]
 * with yxo the unrotated grid (i - (nsamp - 1) / 2), two products and one sum per element as np.tensordot forms them.
 * cardinal / yxco [count][2][nsamp][nsamp] follow `memspace`; 8 numbers per PSF group and exposure are uploaded. */
int imcom_affine_positions(imcom_ctx *ctx, int count, const double *cardinal, int nsamp, double *yxco, int memspace);
/* OutPSF.psf_gaussian psfutil.py:117-146 and OutPSF.psf_simple_airy 148-223 (n x n, row-major) */
int imcom_psf_gaussian(imcom_ctx *ctx, int n, double sigmax, double sigmay, double *out, int memspace);
int imcom_psf_simple_airy(imcom_ctx *ctx, int n, double ldp, double obsc, double tophat_conv, double sigma,
                          double *out, int memspace);

/* InImage.smooth_and_pad (reference src/pyimcom/coadd.py:433-474), the smearing of a raw PSF image that
 * InImage.get_psf_pos applies before the image reaches PSFGrp (coadd.py:603-640): zero-pad by
 * npad = imcom_smooth_pad_width() = ceil(tophatwidth + 6 gaussiansigma + 1) rounded up to a multiple of 4 on every
 * side, then convolve (circularly on the padded grid, as the reference's FFT product does) with a top-hat of width
 * tophatwidth and a Gaussian of sigma gaussiansigma, both in pixels of the array.
 *   in  [n][ny][nx]                       out [n][ny + 2 npad][nx + 2 npad]      (host or device, memspace) */
int imcom_smooth_pad_width(double tophatwidth, double gaussiansigma);
int imcom_smooth_and_pad(imcom_ctx *ctx, int n, const double *in, int ny, int nx, double tophatwidth, double gaussiansigma,
                         double *out, int memspace);

/* PSFGrp.accel_pad_and_rfft2 + PSFOvl._build_psfovl (psfutil.py:943-986, 1244-1294): correlation
 * tables out[p][q] = irfft2(rft(psf1[p]) * conj(rft(psf2[q]))), rolled by nc and cropped to
 * nsamp x nsamp.  psf1[n1][nsamp][nsamp], psf2[n2][nsamp][nsamp]; pairs[npairs][2] HOST lists the
 * (p,q) wanted, tables[npairs][nsamp+12][nsamp+12] (zero border included).
 * amp_penalty HOST: NULL, or {cfg.amp_penalty[0], cfg.amp_penalty[1] * oversamp}: both groups' spectra are
 * reweighted by 1 + a0 exp(-2 pi^2 |u|^2 a1^2) as PSFGrp.__init__ does (psfutil.py:661-671). */
int imcom_psf_overlap(imcom_ctx *ctx, const double *psf1, int n1, const double *psf2, int n2,
                      int nsamp, int nfft, const int *pairs_host, int npairs, const double *amp_penalty,
                      double *tables);

/* The two halves of imcom_psf_overlap, for callers that keep the forward spectra of a PSF group resident and cross
 * them with several other groups (SysMatA builds PSFOvl(grp1, grp2) for every pair of neighbouring 2x2 groups from
 * the same PSFGrp.psf_rft, psfutil.py:1904-2010, 943-986):
 *   imcom_psf_spectra_size   doubles per PSF of a spectra buffer, or 0 when nfft has no butterfly plan (other prime
 *                            factors than 2, 3, 5, or > 1024) -- then only imcom_psf_overlap (dense-DFT form) serves
 *   imcom_psf_spectra        spectra[n][size] (DEVICE) = rfft2 of the zero-padded PSFs psf[n][nsamp][nsamp] (DEVICE)
 *   imcom_psf_overlap_spectra  tables[npairs][nsamp+12][nsamp+12] (DEVICE) exactly as imcom_psf_overlap, from spectra;
 *                            pairs (HOST) index spec1 / spec2
 *   imcom_psf_overlap_spectra_win  the same with a window per pair, win (HOST) [npairs][4] = {row_lo, row_hi, col_lo, col_hi} in
 *                            window coordinates 0..nsamp (table row = 6 + window row), or NULL: only that part of a table
 *                            (and the zero border next to it) is guaranteed to be written.  For the cross tables of two
 *                            PSF groups that own disjoint ranges of InStamp cells (SysMatA.ji_st2psf, psfutil.py:1803-1824):
 *                            the separations between their pixels have one sign along every axis in which the groups
 *                            differ, so half (a quarter) of such a table is never interpolated (psfutil.py:1401-1495). */
long imcom_psf_spectra_size(int nsamp, int nfft);
int imcom_psf_spectra(imcom_ctx *ctx, const double *psf, int n, int nsamp, int nfft, double *spectra);
int imcom_psf_overlap_spectra(imcom_ctx *ctx, const double *spec1, int n1, const double *spec2, int n2, int nsamp, int nfft,
                              const int *pairs, int npairs, const double *amp_penalty, double *tables);
int imcom_psf_overlap_spectra_win(imcom_ctx *ctx, const double *spec1, int n1, const double *spec2, int n2, int nsamp, int nfft,
                                  const int *pairs, int npairs, const double *amp_penalty, const int *win, double *tables);
/*   imcom_psf_overlap_spectra_slots  the same into an ARENA of tables: slots (HOST) [npairs] = index of the arena table that
 *                            receives pair t's result, `tables` = the arena's first table, nslots its size (range check).
 *                            A block keeps the PSFOvl sets of the PSF groups it is working on resident and replaces the least
 *                            recently used ones (the reference's reference-counted SysMatA cache, psfutil.py:1868-1902,
 *                            2012-2092): freed tables are reused one by one, so a set need not be contiguous. */
int imcom_psf_overlap_spectra_slots(imcom_ctx *ctx, const double *spec1, int n1, const double *spec2, int n2, int nsamp, int nfft,
                                    const int *pairs, int npairs, const double *amp_penalty, const int *win, const int *slots,
                                    int nslots, double *tables);
/* PSFSPLIT (PSFGrp.setup(psfsplit=True), PSFOvl.setup psfutil.py:1087-1089): the overlap tables are wider than the PSFs --
 * PSFOvl.nsamp = 2 * PSFGrp.nsamp + 1 = nfft - 1, PSFOvl.nc = PSFGrp.nsamp -- i.e. roll(irfft2(R1 conj R2), nc)[: 2 nc + 1, : 2 nc + 1]
 * (1226-1227) is the whole cyclic correlation but one row and one column.  The entries below take the table side `ntab` (odd,
 * nsamp <= ntab <= nfft - 1; rolled by ntab / 2) beside the PSF side `nsamp`; ntab == nsamp computes what the plain entries compute.
 *   imcom_psf_overlap_wide          as imcom_psf_overlap (any nfft: butterfly plan or dense DFT): tables[npairs][ntab+12][ntab+12]
 *   imcom_psf_overlap_spectra_wide  as imcom_psf_overlap_spectra_slots from the spectra of imcom_psf_spectra (which do not depend on the
 *                            table side): win [npairs][4] in table coordinates 0..ntab or NULL, slots [npairs] or NULL (then pair t goes
 *                            to tables[t]), tables of (ntab+12)^2 doubles each.  The intermediate of the two inverse transforms
 *                            ((ntab + 1) x (nfft/2 + 1) complex per pair) is chunked against ~4 GB as for the plain entries. */
int imcom_psf_overlap_wide(imcom_ctx *ctx, const double *psf1, int n1, const double *psf2, int n2, int nsamp, int ntab, int nfft,
                           const int *pairs_host, int npairs, const double *amp_penalty, double *tables);
int imcom_psf_overlap_spectra_wide(imcom_ctx *ctx, const double *spec1, int n1, const double *spec2, int n2, int nsamp, int ntab,
                                   int nfft, const int *pairs, int npairs, const double *amp_penalty, const int *win, const int *slots,
                                   int nslots, double *tables);

/* pyimcom.meta.ginterp (reference src/pyimcom/meta/ginterp.py), the deconvolution-shear-reconvolution resampler of
 * MetaMosaic.shearimage (meta/distortimage.py:393-593).  Rsearch is served while the offsets number NN <= 320 and the corner
 * system n_g <= 256 (Rsearch 8: 232 / 197); beyond that IMCOM_ERR_UNSUPPORTED.
 *   imcom_ginterp_geometry   (host only, ginterp.py:62-83, 157-159) the NN grid offsets within the search radius in the reference's
 *                            order (row-major meshgrid, filtered) and the corner subsets: posx, posy [NN], corners [4][n_g] = indices
 *                            into posx.  With posx = posy = corners = NULL only NN and n_g; otherwise cap >= NN.
 *   imcom_ginterp_matrix     InterpMatrix (ginterp.py:19-186): T [npts][NN], U and Sigma [ceil(npts / stest)] for the fractional
 *                            positions x_out, y_out [npts].  Cov (HOST) [3] = Cxx, Cxy, Cyy.  Ad of corner 0 is factored once on the
 *                            device (the library's blocked Cholesky), every point is solved by blocked substitution.
 *   imcom_ginterp_resample   MultiInterp (ginterp.py:189-340) fused: output pixel i = y nx + x of an [ny][nx] grid maps to
 *                            (x_in, y_in) = transform (HOST, [2][2] row-major) (x, y) + origin (HOST [2]); in [nlayer][ny_in][nx_in]
 *                            float32 (in_f64 = 0) or float64 (1), in_mask [ny_in][nx_in] (1 = masked) -> out [nlayer][ny][nx] in the
 *                            input's type, out_mask [ny][nx], UmaxSmax [2] over the points whose index within their `blocksize` chunk
 *                            is a multiple of stest.  T exists only per tile of 16 points.  2 bb >= min(nx_in, ny_in): all zeros,
 *                            all masked, Umax = Smax = 0 (the reference's early exit).  A position that is not finite or lies
 *                            beyond the int32 range is masked, as the reference's int32 cast masks it; nothing outside `in` is read.
 *                            Rsearch that is not finite or not positive: IMCOM_ERR_ARG, checked before the geometry is built.
 *   in/out arrays follow `memspace`. */
int imcom_ginterp_geometry(double Rsearch, int cap, int *NN, int *ng, int *posx, int *posy, int *corners);
int imcom_ginterp_matrix(imcom_ctx *ctx, double Rsearch, double samp, int npts, const double *x_out, const double *y_out,
                         const double *Cov, double epsilon, int stest, double *T, double *U, double *Sigma, int memspace);
int imcom_ginterp_resample(imcom_ctx *ctx, int nlayer, int ny_in, int nx_in, const void *in, int in_f64, const unsigned char *in_mask,
                           int ny, int nx, const double *origin, const double *transform, double Rsearch, double samp,
                           const double *Cov, double epsilon, int stest, long blocksize, void *out, unsigned char *out_mask,
                           double *UmaxSmax, int memspace);

/* Injected point-source layers (reference src/pyimcom/layer.py:792-854, GridInject.make_image_from_grid: the image of `cstar`, and the
 * brightness of `nstar`, layer.py:1346-1388).
 *   imcom_psf_from_cube   the draw PSFs of InImage.get_psf_pos for the Legendre-cube formats (coadd.py:624-640) at a batch of positions:
 *                         out[s] = scale * smooth_and_pad(sum_a lpoly[s][a] cube[a], tophatwidth, gaussiansigma), cube [na][ny][nx],
 *                         lpoly [nstar][na] (InImage.LPolyArr, coadd.py:476-510), out [nstar][ny + 2 npad][nx + 2 npad] with npad =
 *                         imcom_smooth_pad_width(); scale = 1/64 for `anlsim`, 1 for `L2_2506` (coadd.py:628-640).  The smearing is linear
 *                         and is applied to the na planes once per call; a star costs the contraction alone (rounding differs).
 *   imcom_draw_stars      layer.py:825-852: for every star s at (xsca[s], ysca[s]) (may lie off the chip) and every native pixel of its
 *                         box [int(x) - d, int(x) + d) x [int(y) - d, int(y) + d) clipped to the image (int() truncates towards zero),
 *                         image[iy][ix] += oversamp^2 * iD5512C(psfs[s] zero-padded by 6) at
 *                         (oversamp (ix - x) + (px - 1)/2 + 6, oversamp (iy - y) + (py - 1)/2 + 6); points off the interpolation grid add
 *                         nothing (routine.py:166-167).  psfs [nstar][py][px], image [nside][nside].  Every pixel adds its stars in
 *                         ascending s, without atomics: the image is the same bit for bit for every split of the star list into calls.
 *   all arrays follow `memspace`. */
int imcom_psf_from_cube(imcom_ctx *ctx, int na, const double *cube, int ny, int nx, int nstar, const double *lpoly, double tophatwidth,
                        double gaussiansigma, double scale, double *out, int memspace);
int imcom_draw_stars(imcom_ctx *ctx, int nstar, const double *psfs, int py, int px, const double *xsca, const double *ysca, double oversamp,
                     int d, int nside, double *image, int memspace);

/* The long-range PSF part of an SCA image (reference src/pyimcom/splitpsf/imsubtract.py, run_imsubtract_single).  s = oversamp, ax = the
 * side of the kernel planes, nside = the side of the SCA, Nl = the Legendre order used (imsubtract.py:482-485).
 *   imcom_imsub_sizes     imsubtract.py:387-389, 451 and the layout of the prepared kernel: out[6] = {I_pad, first_index, A, np = ax / s,
 *                         npp = np rounded up to 8, Nl^2 s^2 np npp = the doubles of the prepared kernel}.  IMCOM_ERR_ARG unless s >= 2,
 *                         ax >= s, nside >= 1, Nl >= 1 and ax is a multiple of 2 s (imsubtract.py:365-366) or, for the kernels that
 *                         bin2x2 trims (imsubtract.py:373-376), s is odd and ax a multiple of s.
 *   imcom_imsub_prepare_kernel_f32   the Nl^2 planes K[0 .. Nl^2-1] of K [ncoeff][ax][ax] (float32; the plane of a term is lu + lv Nl with
 *                         the Nl used, imsubtract.py:698) split into their s^2 phases, flipped and widened: kf [Nl^2][s][s][np][npp]
 *                         doubles in DEVICE memory whatever `memspace` says of K -- the operand that stays resident over the layers of an
 *                         SCA.  IMCOM_ERR_ARG when Nl^2 > ncoeff.
 *   imcom_imsub_canvas_add_f32       imsubtract.py:665-682: canvas[row0 + j][col0 + i] += H[j][i] * area[j / s][i / s] for the hh x hw
 *                         (multiples of s) float64 block H and the float32 native-pixel areas area [hh / s][hw / s]; canvas [A][A] float32.
 *   imcom_imsub_convolve_subtract_f32   imsubtract.py:689-707 for the rows y0 .. y0 + ny - 1 of one layer, without the full-resolution KH:
 *                           image[Y - y0][X] -= sum_c sum_{j,i < ax} K[c][j][i] arr_c[first_index + s Y + ax-1 - j][first_index + s X + ax-1 - i]
 *                         with arr_c = canvas * f32(P_lu(u_x)) * f32(P_lv(u_y)) in float32 (imsubtract.py:487-488, 694-696), c = lu + lv Nl.
 *                         canvas holds the rows crow0 .. crow0 + crows - 1 of the [A][A] canvas and must cover the rows
 *                         first_index + s y0 .. first_index + s (y0 + ny - 1) + ax - 1 the call reads.  kf: the prepared kernel (device
 *                         memory) or NULL, then K is prepared into the workspace by this call.  image [ny][nside] float32 in / out;
 *                         kh (may be NULL) [ny][nside] doubles receives the sums.  Every sample has one owner thread and a fixed order
 *                         of terms, sums are float64: the result is the same bit for bit for every split of the rows into calls.
 *   canvas, K, H, area, image and kh follow `memspace`. */
int imcom_imsub_sizes(int ax, int s, int nside, int Nl, long *out);
int imcom_imsub_prepare_kernel_f32(imcom_ctx *ctx, const float *K, int ncoeff, int ax, int Nl, int s, double *kf, int memspace);
int imcom_imsub_canvas_add_f32(imcom_ctx *ctx, float *canvas, int A, const double *H, int hh, int hw, const float *area, int s, int row0,
                               int col0, int memspace);
int imcom_imsub_convolve_subtract_f32(imcom_ctx *ctx, const float *canvas, int A, long crow0, long crows, const float *K, const double *kf,
                                      int ncoeff, int ax, int Nl, int s, int nside, int y0, int ny, float *image, double *kh, int memspace);

/* The split of a Legendre PSF cube into a short-range PSF and a long-range kernel (reference src/pyimcom/splitpsf/splitpsf.py, class
 * SplitPSF).  n = the side of the cube's planes, npoly = (lorder + 1)^2 planes, plane a = l_y (lorder + 1) + l_x.  Transforms of side
 * N <= 1024 with N a product of 2, 3, 5 run as wave-per-line butterflies (route 1), every other side up to 4096 as dense DFTs on the
 * fp64 MFMA tile engine (route 2): the same formula either way.  A side beyond 4096 (a cube side beyond 2048 in imcom_splitpsf_points):
 * IMCOM_ERR_UNSUPPORTED.
 *   imcom_splitpsf_sizes    out[6] = {npad of tophatfilter (splitpsf.py:134-135), n + 2 npad, the route of the tophat filter's transforms,
 *                           the route of the 2n transforms of imcom_splitpsf_points (0: not served), the workspace bytes of
 *                           imcom_splitpsf_tophat for npoly planes, the workspace bytes of imcom_splitpsf_points for nsca SCAs and npts grid
 *                           points with device pointers and K_real = NULL}.
 *   imcom_splitpsf_tophat   splitpsf.py:131-154: out = the planes of cube [nplane][n][n] smoothed with a tophat of `width` samples: zero
 *                           pad by npad, cyclic 2-D transform, times sinc(u_x width) sinc(u_y width), inverse, crop.  out may be cube.
 *   imcom_splitpsf_split    splitpsf.py:92-128, 223-234: smallpsf [npoly][ns][ns] = W * cube trimmed by (n - ns) / 2 and
 *                           resid [npoly][n][n] = cube * (1 - W) * Trunc, W = Window_2D_integratedBlackman(n, r_in, r_out) (radii in
 *                           samples: oversamp * r_in of the reference), Trunc = Truncate_2D_integratedBlackman(n, m_trunc).  n, ns even
 *                           (IMCOM_ERR_ARG otherwise, as the reference's ValueError).
 *   imcom_splitpsf_points   splitpsf.py:253-284 for the grid points i0 .. i0 + npts - 1 of nsca SCAs at once: locLRP = sum_a lpw[i][a]
 *                           resid[s][a] (267); K_real = gauss_deconv(locLRP, cov[s][i], eps) (156-170); zeta_real = locLRP -
 *                           convolve(K_real, gauss_stamp(n, cov[s][i]), "same") (172-185, 269-274); K_Legendre[s][a] += wg[i] lpw[i][a]
 *                           K_real (277) in ascending i, every element by one owner thread, products and sums rounded one by one; the call
 *                           that holds grid point 0 starts from zero, the one that holds the last applies (l_x + 1/2)(l_y + 1/2)
 *                           (282-284).  The result is the same bit for bit for every split of grid points and SCAs into calls (calls of
 *                           one SCA in ascending i0).  resid, K_Legendre [nsca][npoly][n][n]; K_real, zeta_real (each may be NULL)
 *                           [nsca][npts][n][n]; zetamax [nsca] = max |zeta_real| over the grid points so far (365).  lpw [npoly][npoly]
 *                           (row i: outer(P(y_i), P(x_i)).flatten(), 263-265), wg [npoly] and cov [nsca][npoly][2][2] are HOST arrays
 *                           whatever `memspace` says.  IMCOM_ERR_ARG: npoly not a square, n odd, a covariance that is not positive
 *                           definite (of its off-diagonal elements C[0][1] is the one read, as in the reference).
 *   cube, out, smallpsf, resid, K_Legendre, K_real, zeta_real and zetamax follow `memspace`. */
int imcom_splitpsf_sizes(int n, int npoly, double width, int nsca, int npts, long *out);
int imcom_splitpsf_tophat(imcom_ctx *ctx, const double *cube, int nplane, int n, double width, double *out, int memspace);
int imcom_splitpsf_split(imcom_ctx *ctx, const double *cube, int npoly, int n, int ns, double r_in, double r_out, int m_trunc, double *smallpsf,
                         double *resid, int memspace);
int imcom_splitpsf_points(imcom_ctx *ctx, const double *resid, int nsca, int npoly, int n, int i0, int npts, const double *lpw, const double *wg,
                          const double *cov, double eps, double *K_Legendre, double *K_real, double *zeta_real, double *zetamax, int memspace);

/* Destriping: the cost function and its gradient over a mosaic resident on the device (reference src/pyimcom/imdestripe.py).  Every
 * array is DEVICE memory except the pair table (pair_a .. pair_lat, host arrays of npairs entries).  n_sca SCAs of side nside are stacked:
 * image, g_eff float32 [n_sca][nside][nside], mask bytes (0 / 1), N_eff float64, psi float32; params and the residuals float64
 * [n_sca][nbins], nbins = ds_rows + nside / amp_cols (amp_cols <= 0: rows only).  Ordered pair i gathers neighbour pair_b[i] onto target
 * pair_a[i]; the table is sorted by (a, b) -- the order the sums of a target pixel are formed in, whatever order the caller learnt the pairs
 * in.  The positions of a's pixels in b are pair_x[i], pair_y[i] (float64 [nside][nside]: column and row in b, the x_target, y_target of
 * compareutils.map_sca2sca) or, with both NULL, pair_lat[i] = their values [2][L][L] (x plane, y plane) on the L x L Chebyshev-Lobatto
 * lattice over a's pixel range (row node, column node) with W [nside][L] the Lagrange weights of the nodes at every pixel index: the
 * kernels contract the row axis once per image row and spend L multiply-adds per pixel and coordinate, as imcom_lattice_positions does.
 * The cell is floor; a target pixel whose cell is not wholly inside the source contributes nothing.
 * Seam 21: with pair_x[i], pair_y[i] and pair_lat[i] all NULL the positions of pair i are FORMED in the kernels from the WCSs of its two
 * SCAs and nothing of the grid's size is kept: wcs_desc (DEVICE, float64 [n_sca][130], the packed descriptor of every SCA in the layout
 * stated at imcom_wcs_*; the rows of SCAs no formed pair names are not read), the error tables as five HOST arrays indexed by SCA (tab[s] a
 * DEVICE pointer or NULL, tab_f64, tab_n2, tab_lo, tab_hi as imcom_wcs_* take them; all five NULL: no SCA has one) and pair_M (DEVICE, float64
 * [npairs][9]: row i = R_b R_a^T of imcom_destripe_pair_rotation; read for formed pairs only).  The position of pixel (row r, column c) is
 * imcom_wcs_pix2pix's of the point (c, r), origin 0, with its NaN rule -- the same arithmetic in the same order, so the same bits as the
 * arrays that entry would have stored.  A mosaic may mix the three sources pair by pair.  All seven NULL: no pair is formed.
 *   imcom_destripe_wcs_sizes out[4] = {bytes kept for one formed pair (its row of pair_M), bytes of wcs_desc for n_sca SCAs, doubles of a
 *                            descriptor, workspace bytes of imcom_wcs_effective_gain for an SCA of this side}.
 *   imcom_destripe_pair_rotation   M [9] (HOST) = R_ref R_target^T of two packed descriptors (HOST) after their refusals.
 *   imcom_destripe_sizes     out[8] = {nbins, column blocks, resident bytes per SCA (image, mask, g_eff, N_eff, psi), bytes of a pair's
 *                            position arrays, bytes of a pair's lattice, workspace bytes of imcom_destripe_cost, of imcom_destripe_residual,
 *                            bytes of W}.  IMCOM_ERR_UNSUPPORTED: ds_rows != nside (the "linear" model's 2 ds_rows parameters cannot be
 *                            broadcast by the reference's own forward_par, imdestripe.py:690-691), amp_cols that does not divide nside
 *                            (643-648), L outside 2 .. 33, a shape whose bins do not fit a workgroup's LDS.
 *   imcom_destripe_neff      N_eff[a] = sum_b Interp_{b->a}[mask_b] (Sca_img.make_interpolated 535-562; once per mosaic).
 *   imcom_destripe_cost      make_interpolated 476-594, interpolate_image_bilinear 972-998, subtract_parameters 430-449, apply_all_mask
 *                            421-427, Parameters.forward_par 670-703, cost_function_single 1546-1559, the cost models 875-887,
 *                            compute_boundary_continuity_penalty 1413-1489:  J_a = sum_b Interp_{b->a}[(I_b - P_b) mask_b g_b] (NaN -> 0, the
 *                            stripe image P_b never formed), new_mask = N_eff > neff_min, J_a = where(new_mask, J_a / N_eff, 0) / g_a,
 *                            psi = where(new_mask mask_a, (I_a - P_a) mask_a - J_a, 0) rounded once to float32,
 *                            eps[a] = sum f(psi) (+ col_boundary_const * penalty when amp_cols > 0 and col_boundary_const > 0; amp_cols < 50
 *                            is then IMCOM_ERR_UNSUPPORTED) in float64, rows in a fixed tree, then in row order.
 *   imcom_destripe_residual  residual_function 1311-1317, residual_function_single 1375-1403, transpose_interpolate 1001-1023,
 *                            transpose_par 1026-1058, the derivatives 890-902:  g = f'(psi), term_1 = the row (and column-block) sums of g;
 *                            g /= g_a N_eff where N_eff != 0, else 0; every target pixel adds its four weighted values times g_b at the
 *                            corners to the bins of b (gradient_original is never formed).  resids = term_2 - term_1; resids1 = -term_1
 *                            and resids2 = term_2 when not NULL.  term_2 is summed as fixed-point integers of one scale per call (2^e with
 *                            n_sca nside^2 max|g| geff_max < 2^(62-e); geff_max >= max g_eff): exact sums of once-rounded terms, the same
 *                            bits for every order of arrival.
 *   imcom_destripe_interp / _transpose   the two routines on their own for float64 images: out[i] += the bilinear value of src * gsrc
 *                            [rows][cols] at (x[i], y[i]); out [rows][cols] += the transposed scatter of image[i]. */
#define IMCOM_DESTRIPE_QUADRATIC 0
#define IMCOM_DESTRIPE_ABSOLUTE 1
#define IMCOM_DESTRIPE_HUBER 2
int imcom_destripe_sizes(int n_sca, int nside, int ds_rows, int amp_cols, int L, int max_np, int npairs, long *out);
int imcom_destripe_neff(imcom_ctx *ctx, int n_sca, int nside, int L, const unsigned char *mask, int npairs, const int *pair_a, const int *pair_b,
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, double *neff,
                        const double *wcs_desc, const void *const *tab, const int *tab_f64, const int *tab_n2, const double *tab_lo, const double *tab_hi,
                        const double *pair_M);
int imcom_destripe_cost(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *image, const unsigned char *mask,
                        const float *geff, const double *neff, const double *params, int npairs, const int *pair_a, const int *pair_b,
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, int model, double thresh,
                        double neff_min, double col_boundary_const, float *psi, double *eps, const double *wcs_desc, const void *const *tab, const int *tab_f64,
                        const int *tab_n2, const double *tab_lo, const double *tab_hi, const double *pair_M);
int imcom_destripe_residual(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *psi, const float *geff, const double *neff,
                            int npairs, const int *pair_a, const int *pair_b, const void *const *pair_x, const void *const *pair_y,
                            const void *const *pair_lat, const double *W, int model, double thresh, double geff_max, double *resids, double *resids1,
                            double *resids2, const double *wcs_desc, const void *const *tab, const int *tab_f64, const int *tab_n2, const double *tab_lo,
                            const double *tab_hi, const double *pair_M);
int imcom_destripe_wcs_sizes(int n_sca, int nside, long *out);
int imcom_destripe_pair_rotation(const double *target, const double *ref, double *M);
int imcom_destripe_interp(imcom_ctx *ctx, const double *src, const double *gsrc, int rows, int cols, const double *x, const double *y, long npix, double *out);
int imcom_destripe_interp_transpose(imcom_ctx *ctx, const double *image, const double *x, const double *y, long npix, int rows, int cols, double *out);

/* Noise power spectra of coadded frames (reference src/pyimcom/analysis.py, NoiseAnal.__call__ 745-807 and the loop of
 * _BlkGrp.get_noise_power_spectra 1270-1303; src/pyimcom/diagnostics/noise_diagnostics.py, NoiseReport.measure_power_spectrum 400-443 and
 * azimuthal_average 472-506).  Frames are real, of even side L <= 4096, float32 or float64 (in_f64); the arithmetic is float64 throughout.
 * A frame's result depends on that frame only (rows 2j, 2j+1 of ONE frame ride as a complex line), every output element has one owner
 * thread and a fixed summation order: the same bits from run to run and however frames are grouped into calls.  Routes of the line
 * transforms: 1 the wave-per-line butterflies (L <= 1024 a product of 2, 3, 5), 3 two-level (L = N1 N2, N1 a butterfly side, 2 <= N2 <= 16:
 * 2560 = 640 x 4, 2688 = 384 x 7), 2 the dense DFT on the fp64 MFMA tile engine (every other side; IMCOM_NOISEPS_ROUTE=dense in the
 * environment forces it).  IMCOM_ERR_ARG: L odd, L % 8 != 0 with bin8, L > 4096, a window that is not L x L, a route that does not serve L.
 *   imcom_noiseps_route      the route of side L (0: not served).  Returns the route, not a status.
 *   imcom_noiseps_sizes      out[4] = {route served (argument route = 0: the plan's choice), side of an output frame (L / 8 with bin8, else L),
 *                            workspace bytes of imcom_noiseps_2d for nframe frames with device pointers, bytes of one frame's half spectrum}.
 *   imcom_noiseps_2d         analysis.py:789-794 / noise_diagnostics.py:430-441: out[f][ky][kx] = |F_f[(ky - L/2) mod L][(kx - L/2) mod L]|^2
 *                            / norm[f], F_f the 2-D transform of frame f times `window` (NULL: none; window_len = its element count, L L),
 *                            i.e. the fftshift-ed full spectrum, its missing half by Hermitian symmetry; with bin8 the 8 x 8 averages (sum,
 *                            then one division by 64), out [nframe][L/8][L/8], else [nframe][L][L].  Element (f, y, x) of `frames` is at
 *                            f fstride + y rstride + x (in elements): a cropped view of a larger block is read in place.  norm [nframe] is a
 *                            HOST array whatever `memspace` says; with a window the caller passes norm * mean(window^2) (432).
 *   imcom_noiseps_radial     analysis.py:699-702 (ndimage.mean, standard_deviation, sum over labels): for index i = 1 .. nidx of the int32
 *                            labels rbin [n][n], mean[f][i-1] over the pixels of image [nframe][n][n] with that label and err[f][i-1] =
 *                            sqrt(sum (x - mean)^2 / npix) / sqrt(npix), two passes.  One pixel: err = 0 exactly; none: NaN (as ndimage).
 *   imcom_noiseps_accumulate analysis.py:1278-1279 on the device, in call order: ps2d_all [nlayers][n][n] += ps2d [nlayers][n][n];
 *                            ps1d_all [nlayers][bins][nrad][2] at coverage_bin += (mean, err) [nlayers][nrad].  DEVICE memory throughout.
 *   frames, window, out, image, rbin, mean and err follow `memspace`. */
int imcom_noiseps_route(int L);
int imcom_noiseps_sizes(int L, int nframe, int bin8, int route, long *out);
int imcom_noiseps_2d(imcom_ctx *ctx, const void *frames, int in_f64, int nframe, int L, long fstride, long rstride, const double *window, long window_len,
                     const double *norm, int bin8, int route, double *out, int memspace);
int imcom_noiseps_radial(imcom_ctx *ctx, const double *image, int nframe, int n, const int *rbin, int nidx, double *mean, double *err, int memspace);
int imcom_noiseps_accumulate(imcom_ctx *ctx, const double *ps2d, const double *mean, const double *err, int nlayers, int n, int nrad, int bins, int coverage_bin,
                             double *ps2d_all, double *ps1d_all);

/* Draws of numpy's PCG64 stream by position, and the simulated cosmic-ray mask made of them (reference src/pyimcom/layer.py:933-964,
 * Mask.randmask; 1071-1077, the lab-noise threshold of Mask.load_cr_mask; 313-401, GalSimInject.subgen / subgen_multirow).  The stream is
 * given as numpy reports it, np.random.PCG64(seed).state["state"]: `state` and `inc`, each as its low and high 64 bits; seeding stays
 * numpy's.  U[k], k = 0, 1, ..., is the double that Generator.random() / uniform() returns as draw k + 1 from that state: the state moved
 * k + 1 steps of s <- 0x2360ED051FC65DA44385DF649FCCF645 s + inc (mod 2^128), the output rotr64(hi ^ lo, s >> 122), and (output >> 11)
 * 2^-53.  Integer arithmetic until that one exact conversion: every result equals numpy's bit for bit, whatever the count, the offset
 * and the memspace.  These entries serve draws that consume one 64-bit output each; normal draws are imcom_pcg64_normal's, below.
 *   imcom_pcg64_uniform     out[i] = U[offset + i], i < count; offset = offset_hi 2^64 + offset_lo.  IMCOM_ERR_ARG: count < 0.
 *   imcom_pcg64_uniform_at  out[i] = U[pos[i]], i < count; pos int64 in any order (an entry below 0 counts as its value mod 2^64).
 *   imcom_cr_mask           Mask.randmask: pixel (r, c) of slice `slice` (idsca[1] - 1) of the padded draw [n_slices][W][W], W = nside +
 *                           2 pad (the reference: n_slices 18, pad 10, nside 4088), is U[slice W^2 + r W + c]; it is a hit when
 *                           U < pcut (float64).  mask [nside][nside] uint8: 1 where none of the nine padded pixels around (y + pad,
 *                           x + pad) is a hit, else 0.  With labnoise [nside][nside] float32 (NULL: none) also layer.py:1076: mask &=
 *                           |labnoise| < threshold, compared in float64 (the caller rounds `threshold` to the type numpy would compare
 *                           in; a NaN pixel is masked).  *ngood: the number of 1s.  No image of draws is formed: hits live in LDS.
 *                           IMCOM_ERR_ARG: nside outside 1 .. 65536, pad outside 1 .. 4096, n_slices outside 1 .. 65536, slice outside
 *                           0 .. n_slices - 1.
 *   pos, out, labnoise, mask and ngood follow `memspace`. */
int imcom_pcg64_uniform(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                        long count, double *out, int memspace);
int imcom_pcg64_uniform_at(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, const long *pos, long count, double *out,
                           int memspace);
int imcom_cr_mask(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, int nside, int pad, int slice, int n_slices,
                  double pcut, const float *labnoise, double threshold, unsigned char *mask, long *ngood, int memspace);

/* numpy's float64 normal draws of a PCG64 stream (Generator.standard_normal / normal; reference src/pyimcom/layer.py:1303-1304, the
 * white-noise layer drawn for every input image, and 899-900, the draws of CplxNoise.noise_1f_frame).  The stream is given as for
 * imcom_pcg64_uniform.  A normal draw takes one stream output 99.3 % of the time and more otherwise (a ziggurat: csrc/ziggurat_core.h), so
 * draw i has no stream position of its own; the draws are found as a chain through the stream, tile by tile (csrc/ziggurat.hip).
 *   imcom_pcg64_normal_sizes  *tail_cap: the entries tail_idx must have room for (tail_raw: twice as many) for `count` draws.
 *   imcom_pcg64_normal        out[i], i < count: the draws Generator.standard_normal(count) returns after bit_generator.advance(offset),
 *                             bit for bit, EXCEPT the tail draws (|x| > 3.654, 2.7e-4 of all).  A tail draw's last bit depends on the
 *                             libm numpy was built against, so for those out[i] is NOT final: it holds this library's log1p, which may
 *                             differ from numpy's in the last bit, and nothing in `info` says whether it does.  A caller that wants
 *                             numpy's bits must overwrite them: tail_idx[j] = i, tail_raw[2 j], tail_raw[2 j + 1], j < info[2], in no
 *                             particular order, are the attempt's first output w0 and the output w1 whose logarithm the value holds,
 *                             x = 3.6541528853610088 - 0.27366123732975828 log1p(-(w1 >> 11) 2^-53), negated if bit 17 of w0 is set,
 *                             formed with the caller's libm.  A caller that ignores the list has normal draws that equal numpy's except
 *                             possibly in the last bit of those entries.  info [4], host memory whatever the memspace: the stream
 *                             outputs the count draws consume (the state numpy is left in is that many steps on), the consumed
 *                             attempts that left the fast path, the tail draws, and 1 if the call is UNDECIDED: a comparison of the
 *                             draw that depends on exp / log1p fell inside the guard band (relative 2^-46; two correct evaluations of
 *                             a side differ by less than 2^-49), a tail loop ran over 8 pairs, or there were more than tail_cap tail
 *                             draws.  Then `out` is not numpy's and the caller draws the request on the host: about one call in 7 10^5
 *                             for 4088^2 draws, two thirds of them from the tail loop (csrc/ziggurat_core.h has the account).  The call
 *                             waits for its work (once per chunk of tiles).  IMCOM_ERR_ARG: count < 0.
 *   imcom_pcg64_normal_ex     the same with, for tests and measurements, the tile size (a power of two, 4 .. 1024), the tiles of one
 *                             chunk (<= 2^20) and the guard band of this call; 0 is the default.  No result depends on the first two.
 *                             IMCOM_ERR_ARG for values outside these ranges.
 *   out, tail_idx and tail_raw follow `memspace`. */
int imcom_pcg64_normal_sizes(long count, long *tail_cap);
int imcom_pcg64_normal(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                       long count, double *out, long *tail_idx, uint64_t *tail_raw, uint64_t *info, int memspace);
int imcom_pcg64_normal_ex(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                          long count, double *out, long *tail_idx, uint64_t *tail_raw, uint64_t *info, int memspace, int tile, long chunk_tiles,
                          double guard_band);

/* numpy's Poisson draws of a PCG64 stream (Generator.poisson(lam = array); reference src/pyimcom/layer.py:1385-1387, the noise of the nstar
 * layer).  The stream is given as for imcom_pcg64_uniform.  A draw of rate 0 consumes nothing, one of 0 < lam < 10 as many outputs as its
 * value plus one, one of lam >= 10 two outputs per attempt of a transformed rejection (csrc/poisson_core.h), so where draw i starts depends
 * on every draw before it and on their rates; the path is found superchunk by superchunk through windows of candidate positions, and a
 * superchunk whose path leaves its windows is redone one draw after another (csrc/poisson.hip).
 *   imcom_pcg64_poisson_sizes  the device workspace a call of `count` draws takes with its arrays in device memory, and the part of it
 *                              that is scratch of one superchunk.
 *   imcom_pcg64_poisson        out[i], i < count (int64): what Generator.poisson(lam = lam[0 .. count)) returns after
 *                              bit_generator.advance(offset), bit for bit.  info [4], host memory whatever the memspace: the stream outputs
 *                              the draws consume (the state numpy is left in is that many steps on); 1 if the call is UNDECIDED: a
 *                              comparison of a draw ON THE PATH that depends on log / exp fell inside the guard band (absolute, 2^-47
 *                              times the summed magnitudes of the terms, for the rejection's logarithmic test; relative 2^-47 for prod >
 *                              exp(-lam)) or a draw ran into its loop cap (32 attempts, 64 outputs) -- then `out` is not numpy's and the
 *                              caller draws the request on the host, at most one 4088^2 frame in 1.2e4 at lam = 86; the superchunks redone
 *                              by the sequential walk; 1 if a rate is negative, NaN or above numpy's POISSON_LAM_MAX: then nothing is
 *                              written and the call returns IMCOM_ERR_ARG.  IMCOM_ERR_ARG also for count < 0.  The call waits for its work.
 *   imcom_pcg64_poisson_ex     the same with, for tests and measurements, the draws of a superchunk (a multiple of `tile`, <= 65536), the
 *                              window (2 .. 4096), the draws of a tile, the guard band (0: none; 1: every comparison undecided) and
 *                              force_walk (every superchunk by the sequential walk).  0 -- for the guard band a negative value -- is the
 *                              default.  No result depends on any of them except through info[1] and info[2].
 *   imcom_nstar_layer          layer.py:1385-1387 for `count` pixels: lam = brightness tot_int + bg, _lam = max(lam, 0), out = ((P - _lam) +
 *                              lam) - bg in float64 in that order, rounded to float32, P the draws of the rates _lam; no int64 frame is
 *                              stored.  info as above.
 *   lam, brightness and out follow `memspace`. */
int imcom_pcg64_poisson_sizes(long count, long *workspace_bytes, long *scratch_bytes);
int imcom_pcg64_poisson(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                        const double *lam, long count, long *out, uint64_t *info, int memspace);
int imcom_pcg64_poisson_ex(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                           const double *lam, long count, long *out, uint64_t *info, int memspace, int superchunk, int window, int tile, double guard_band,
                           int force_walk);
int imcom_nstar_layer(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                      const double *brightness, double tot_int, double bg, long count, float *out, uint64_t *info, int memspace);

/* The transform of the 1/f noise layer (reference src/pyimcom/layer.py:896-913, the channel loop of CplxNoise.noise_1f_frame; the draws of
 * 899-900 are imcom_pcg64_normal's, the amplitudes of 892-895 the caller's).  normals [2 nch][len]: rows 2c, 2c + 1 are the real and the
 * imaginary draws of channel c; amp [len].  Per channel: the forward DFT of (re + i im) amp in float64 (a four-step transform, len = N1 N2),
 * the real part of outputs k < len / 2, divided by sqrt(2), minus the channel mean (summed in float64 in a fixed order), cast to float32
 * into columns c w .. c w + w - 1 of a [len / 2 / w][nch w] frame, the columns of odd channels reversed.  frame [len / 2 / w - 2 border]
 * [nch w - 2 border] float32 is that frame without a border of `border` pixels (the reference: len 2^20, nch 32, w 128, border 4, the
 * slice [4:4092, 4:4092]).  block (NULL: not wanted) [nch][len / 2] float64: the channels before the cast.  The same bits from run to run.
 * IMCOM_ERR_UNSUPPORTED: len no power of two in 2^10 .. 2^20, or w no power of two <= len / 2.  IMCOM_ERR_ARG: nch outside 1 .. 4096, a
 * border that leaves no pixel.  All arrays follow `memspace`. */
int imcom_noise_1f(imcom_ctx *ctx, const double *normals, const double *amp, long len, int nch, int w, int border, float *frame, double *block,
                   int memspace);

/* Bright-object masks of the destripe set-up (reference src/pyimcom/imdestripe.py:781-872, apply_object_mask; its caller
 * Sca_img.__init__ 317-332; apply_jwst_mask 412-419 needs no entry).  Images are float32 or float64 (is_f64), masks and flags uint8 with
 * one byte a pixel (0 / not 0 in, 0 / 1 out).  Every result is a boolean image, a count or an order statistic, formed from comparisons
 * and integer sums: equal to numpy / scipy bit for bit and the same from run to run.  The scalar steps between the calls (817, 834, 845,
 * 852-853, 863: thresholds, 1.4826 mad, the max() and the breaks) are the caller's, in numpy scalars.
 *   imcom_select_kth      np.median / np.partition (817, 832-833, 842-843): order statistics k and min(k + 1, m - 1) of the m values whose
 *                         flag is not 0 (flags NULL: all n), or with k < 0 the two middle ones, ranks (m - 1) / 2 and m / 2, whose mean in
 *                         the array's type is the median.  use_abs: of |v - c| instead, formed in the array's type and never stored
 *                         (the MAD, 833).  NaNs sort last; a rank among them gives NaN.  -0.0 and 0.0 are one value (0.0 is returned).
 *                         out: two values of the array's type; info[2] = {m, number of NaNs among them}; m = 0 gives NaNs.
 *                         Radix select on order-preserving integer keys, digits of 11 bits, histograms in LDS merged with integer adds.
 *                         IMCOM_ERR_ARG: n < 1, k >= n.
 *   imcom_mask_threshold  855-856 and 863: seed = ok && (v - bkg) >= t_seed, and with grow != NULL grow = ok && (v - bkg) >= t_grow in the
 *                         same pass; ok = isfinite(v) with finite_only, else true (863 has no such test: bkg = 0 there).  v - bkg in the
 *                         array's type; the comparison in float64, which is exact for either type (the caller rounds a threshold to
 *                         the type numpy would compare in).
 *   imcom_mask_clip       820 and 837-840: keep_out = keep_in && |v - bkg| < t, or with keep_in NULL keep_out = isfinite(v);
 *                         *count = the number kept.  keep_out may be keep_in.  The reference's clip_vals[keep] is cumulative, so the
 *                         flags of round i + 1 made from those of round i are its subset.
 *   imcom_mask_propagate  857, scipy.ndimage.binary_propagation(seed, mask=grow), default structure (4-connectivity), border 0: out = seed
 *                         plus every grow pixel joined to it by a 4-connected path of grow pixels.  Tiles of 62 x 62 pixels are grown to
 *                         their own fixpoint in LDS; sweeps repeat while one of them changed (*sweeps, a HOST long or NULL: how many
 *                         ran).  No workgroup waits for another; the fixpoint is unique.  out may be seed, not grow.
 *   imcom_mask_dilate     858-860 and 865, binary_dilation with a (2 r + 1) x (2 r + 1) structure of ones, border 0.  3 x 3 twice and then
 *                         5 x 5 is r = 4.  IMCOM_ERR_UNSUPPORTED: r outside 1 .. 8.  IMCOM_ERR_ARG: out == in.
 *   imcom_mask_apply      867-872, out = mask ? 0 : in over n elements of dtype 0 float32, 1 float64, 2 uint8 (330-332: sca_mask &=
 *                         ~object_mask is dtype 2 with in = out = the SCA's mask).  out may be in.
 *   Every array follows `memspace`.  Workspace: the selection's state and histograms (33 KB); the second image of the propagation. */
int imcom_select_kth(imcom_ctx *ctx, const void *values, int is_f64, long n, const unsigned char *flags, int use_abs, double c, long k, void *out, long *info,
                     int memspace);
int imcom_mask_threshold(imcom_ctx *ctx, const void *image, int is_f64, long n, double bkg, double t_seed, double t_grow, int finite_only, unsigned char *seed,
                         unsigned char *grow, int memspace);
int imcom_mask_clip(imcom_ctx *ctx, const void *image, int is_f64, long n, const unsigned char *keep_in, double bkg, double t, unsigned char *keep_out, long *count,
                    int memspace);
int imcom_mask_propagate(imcom_ctx *ctx, const unsigned char *seed, const unsigned char *grow, int rows, int cols, unsigned char *out, long *sweeps, int memspace);
int imcom_mask_dilate(imcom_ctx *ctx, const unsigned char *in, int rows, int cols, int r, unsigned char *out, int memspace);
int imcom_mask_apply(imcom_ctx *ctx, const void *in, int dtype, const unsigned char *mask, long n, void *out, int memspace);

/* Validation-report statistics (reference src/pyimcom/diagnostics/layer_diagnostics.py:24-64 _percentiles_and_delete and 102-177, the
 * gathering loop of LayerReport.build; src/pyimcom/diagnostics/dynrange.py:140-163, the SIGMA / EFFCOVER histograms, and 211-238, the ring
 * profiles of gen_dynrange_data): exact order statistics of data that never sits in one place, for n_segments <= 64 segments and up to
 * n_ranks <= 32 ranks per segment at once, and the histogram of a (u)int16-coded map.  The accumulator is a radix select on
 * imcom_select_kth's keys and digits (float32: 3 passes of 11 / 11 / 10 bits, float64: 6) whose counters live in `state`, DEVICE memory
 * of the caller (imcom_quant_sizes says how much) that must stay untouched until imcom_quant_free.  The caller feeds the SAME multiset of
 * (segment, value) in every pass, in any chunking and order; all counts are 64-bit integers added with atomics, so every result is the
 * same bits from run to run and for every chunking.  NaNs sort last, a rank among them is NaN, -0.0 and 0.0 are one value (0.0).
 *   imcom_quant_sizes        out[4] = {bytes of `state`, passes, counters per group (2048), groups whose counters share a launch (8)}.
 *   imcom_quant_begin        a new accumulator on `state`, ready for pass 1.  imcom_quant_reset: back to there.  imcom_quant_free.
 *   imcom_quant_add_2d       layer_diagnostics.py:139-142: element (r, c) of a strided view, at values[r pitch + c] (in elements), read in
 *                            place, all into `segment`: a block frame's [d:-d, d:-d] crop.  Counters in LDS, 8 live groups a launch.
 *   imcom_quant_add_flat     n values with a segment id each (uint8, or int32 with ids_i32); an id outside 0 .. n_segments - 1 fails the pass.
 *   imcom_quant_add_constant layer_diagnostics.py:114, 122, 133-134 (the zeros a missing block leaves): `count` copies of `value`, no data.
 *   imcom_quant_add_rings    dynrange.py:216-228: for star k at (x[k], y[k]) (float64) every pixel of its clipped box (217-220) of the frame
 *                            [n][n] goes to segment j = floor(sqrt((col - x)^2 + (row - y)^2)) when j < rpix <= n_segments, once per star
 *                            whose box holds it; the radius in float64 as numpy forms it (no fused multiply-add, the correctly rounded
 *                            root).  n <= 32767 and |x|, |y| < 32765 - rpix (the int16 of the reference), else the pass fails.
 *   imcom_quant_end_pass     ends the pass that was fed; *passes_left (may be NULL).  IMCOM_ERR_ARG, reported here and nowhere earlier:
 *                            a segment whose element or NaN count differs from pass 1's, a bad segment id or star position.  The failed
 *                            pass has then not happened: its counters are zero again, it can be fed anew (or imcom_quant_reset).
 *   imcom_quant_counts       after pass 1: total[s] and nans[s] (HOST arrays [n_segments]), NaNs included in total.
 *   imcom_quant_set_ranks    between pass 1 and pass 2: ranks [n_segments][n_ranks] (HOST), 0-based ranks among the segment's elements in
 *                            ascending order, -1 for a slot not used.  IMCOM_ERR_ARG: a rank >= the count of a segment that is not empty.
 *   imcom_quant_results      after the last pass: out [n_segments][n_ranks] (HOST) of the accumulator's type, the order statistics; NaN
 *                            for an unused slot, a rank among the NaNs, an empty segment.
 *   imcom_codehist           dynrange.py:142-150, 155-163 for a map that is still (u)int16 codes (Block.compress_map): counts [nbins + 1]
 *                            (int64): counts[table[code]] += 1 over the view codes[r pitch + c], the code's bit pattern indexing `table`
 *                            [65536] uint8, which the caller makes by evaluating the reference's expression and comparisons on every
 *                            code: t < 128 bin t (t = nbins: off scale high only), 128 <= t < 255 bin t - 128 and off scale high, 255
 *                            neither.  nbins <= 127.  No power is taken on the device.
 *   values, segment_ids, frame, x, y, codes, table and counts follow `memspace`. */
typedef struct imcom_quant imcom_quant;
int imcom_quant_sizes(int n_segments, int n_ranks, int is_f64, long *out);
int imcom_quant_begin(imcom_ctx *ctx, int n_segments, int n_ranks, int is_f64, void *state, size_t state_bytes, imcom_quant **out);
int imcom_quant_reset(imcom_ctx *ctx, imcom_quant *q);
int imcom_quant_free(imcom_ctx *ctx, imcom_quant *q);
int imcom_quant_add_2d(imcom_ctx *ctx, imcom_quant *q, int segment, const void *values, long rows, long cols, long pitch, int memspace);
int imcom_quant_add_flat(imcom_ctx *ctx, imcom_quant *q, const void *values, const void *segment_ids, int ids_i32, long n, int memspace);
int imcom_quant_add_constant(imcom_ctx *ctx, imcom_quant *q, int segment, double value, long count);
int imcom_quant_add_rings(imcom_ctx *ctx, imcom_quant *q, const void *frame, int n, long pitch, const double *x, const double *y, int nstar, int rpix, int memspace);
int imcom_quant_end_pass(imcom_ctx *ctx, imcom_quant *q, int *passes_left);
int imcom_quant_counts(imcom_ctx *ctx, const imcom_quant *q, long *total, long *nans);
int imcom_quant_set_ranks(imcom_ctx *ctx, imcom_quant *q, const long *ranks);
int imcom_quant_results(imcom_ctx *ctx, const imcom_quant *q, void *out);
int imcom_codehist(imcom_ctx *ctx, const void *codes, long rows, long cols, long pitch, const unsigned char *table, int nbins, long *counts, int memspace);

/* The I24 layer codec (reference src/pyimcom/compress/i24.py: I24Cube.to_mode 367-437, i24compress 443-478, i24decompress 481-514, and the
 * helpers lsbf_fwd / lsbf_rev 41-122, diff_fwd / diff_rev 128-181, smallnum_fwd / smallnum_rev 187-237) for a batch of L layers of ny x nx
 * pixels with a parameter record each; scheme 0 is I24A (int32 codes), 1 is I24B (byte planes [nb][ny][nx], nb = (BITKEEP + 7) / 8, least
 * significant first, with REORDER as bit streams).  Every result equals the reference's bit for bit, from run to run: one owner thread an
 * output element, integer arithmetic, float32 steps rounded one by one, the float64 product and sum of 415 rounded separately.
 * Served is ALPHA == 1 only (IMCOM_ERR_UNSUPPORTED otherwise: the power is numpy's float32 pow).  IMCOM_ERR_ARG: VMAX <= VMIN or either not
 * finite, BITKEEP outside 1 .. 24, SOFTBIAS >= 2^24 (0 .. 2^24 - 1 and -1 are served, any other negative value does nothing, as in the
 * reference), ny nx >= 2^31, L outside 1 .. 4096.  A NaN pixel gets code 0 and no table entry: numpy's cast of NaN to int32 on x86-64
 * followed by the clip of 378.  +inf and -inf are overflow entries.
 * EVERY array is DEVICE memory except pars and counts (HOST).  There is no memspace: a layer that has to cross to the host crosses as codes.
 *   imcom_i24_sizes           no context: checks the parameters (the refusals above) and gives out[8] = {bytes of `state`, workspace bytes of
 *                             a compress call, of a decompress call, bytes of one layer of compressed output (the largest nb of the batch),
 *                             tiles a layer, pixels a tile, tile sums a step of the scan, 0}.
 *   imcom_i24_compress        367-386 and 423-437.  frames: float32, pixel (l, y, x) at frames[l layer_stride + y row_stride + x] (in
 *                             elements; a crop of a larger array is read in place).  Layer l of the result at (char *)out + l out_stride
 *                             (bytes).  counts [L] (HOST): the overflow entries of every layer; the call waits for them.  `state` keeps
 *                             what imcom_i24_overflow_fetch needs and must stay untouched until then.
 *   imcom_i24_overflow_fetch  368-375, once the counts are known: the table of layer l, in ascending flat pixel order (np.where's), at
 *                             entries sum(counts[:l]) .. of y / x (int32) and value (float32); frames, pars, state and counts as in the
 *                             compress call, the frames unchanged since.  capacity: entries the three arrays hold; nothing is written at or
 *                             beyond it, nor beyond a layer's count.  IMCOM_ERR_ARG: capacity < sum(counts).
 *   imcom_i24_decompress      388-420.  Layer l of the input at (const char *)in + l in_stride; planes: the first axis of an I24B cube,
 *                             IMCOM_ERR_ARG if it is not nb.  No bit is masked that the reference does not mask.  DIFF: an inclusive
 *                             wrapping prefix sum over the flat image in three launches (tile sums, their scan, the sum inside the tiles);
 *                             no workgroup waits for another.  The overflow table (counts NULL: none) as imcom_i24_overflow_fetch lays it
 *                             out; out[l][y][x] = value.  A position outside the image is not stored and the call returns IMCOM_ERR_ARG
 *                             (it waits for that answer whenever a table is given).  Positions of one layer are unique in tables this
 *                             codec writes; with duplicates which value stays is unspecified.  out: float32 [L][ny][nx]. */
typedef struct {
    double vmin, vmax, alpha; /* float(pars["VMIN"]), float(pars["VMAX"]), float(pars["ALPHA"]) or 1 */
    long softbias;            /* int(pars["SOFTBIAS"]) or 0 */
    int bitkeep, diff, reorder; /* BITKEEP or 24; bool(pars["DIFF"]) or 0; bool(pars["REORDER"]) or 1 */
} imcom_i24_pars;
int imcom_i24_sizes(int L, long ny, long nx, const imcom_i24_pars *pars, int scheme, long *out);
int imcom_i24_compress(imcom_ctx *ctx, const float *frames, long layer_stride, long row_stride, int L, int ny, int nx, const imcom_i24_pars *pars, int scheme,
                       void *out, long out_stride, void *state, size_t state_bytes, long *counts);
int imcom_i24_overflow_fetch(imcom_ctx *ctx, const float *frames, long layer_stride, long row_stride, int L, int ny, int nx, const imcom_i24_pars *pars,
                             const void *state, size_t state_bytes, const long *counts, int *y, int *x, float *value, long capacity);
int imcom_i24_decompress(imcom_ctx *ctx, const void *in, long in_stride, int planes, int scheme, int L, int ny, int nx, const imcom_i24_pars *pars, const int *y,
                         const int *x, const float *value, const long *counts, float *out);

/* The catalog of injected stars (reference src/pyimcom/analysis.py:1000-1057, StarsAnal.__call__; src/pyimcom/diagnostics/
 * starcube_nonoise.py:186-237, gen_starcube_nonoise; psfutil.py:516): per star a cut of a frame, the adaptive-moment iteration on it (the
 * iteration behind GalSim's FindAdaptiveMom -- restated from the published algorithm, not compared with an installed GalSim), the fourth
 * moments and the forced-scale moments over the same cut, and the means of small windows of the maps.  All sums are float64, reduced in a
 * fixed order that does not depend on the number of stars: a star's numbers are the same bits alone and in any batch, run after run.
 * `frame` / `map`: rows x cols elements, `pitch` elements from row to row.  ox, oy (int32 [nstar]): frame column and row of the cut's first
 * pixel, which may lie outside the frame; pixels outside the frame are zero (np.pad).  memspace covers every array but `par`.
 *   imcom_star_sizes         no context: out[4] = {workspace bytes of an imcom_star_moments call with host arrays, the largest side of a
 *                            cut, the result columns a star, LDS bytes of a moments workgroup}.  IMCOM_ERR_UNSUPPORTED: w or h above 127.
 *   imcom_star_moments       out [nstar][22] float64: amp, x, y (1-based cut coordinates, as galsim.Image has them), sigma, e1, e2, g1, g2,
 *                            rho4, iterations, status (0 ok, 1 not positive definite, 2 empty bounds, 3 moment or shift too large, 4 too
 *                            many iterations, 5 NaN), the last convergence factor; then, for status 0 and forced_scale > 0: sum wti, sum wti
 *                            (u^4 - v^4), sum wti (u^3 v + u v^3), sum wti2, sum wti2 (x^2 - y^2), sum wti2 2xy, M42_REAL, M42_IMAG,
 *                            FORCED_PLUS, FORCED_CROSS (1016-1041).  forced_scale <= 0: columns 12-21 stay zero.  par NULL: the defaults.
 *   imcom_star_window_stats  out [nstar][2]: mean and population standard deviation of map[yi+1-bd2 : yi+bd2, xi+1-bd2 : xi+bd2] as numpy
 *                            slices it (clipped at the far edges; NaN for an empty window).  kind 0: float32, 1: float64, 2: 16-bit codes
 *                            looked up in table (int16 [65536], indexed by the code's bit pattern) and summed as integers.
 *   imcom_star_cuts          out float32 [nstar][h][w]: the cuts themselves, zero outside the frame. */
typedef struct {
    double convergence_threshold; /* 1e-6 */
    double bound_correct_wt;      /* 0.25 */
    double max_amoment;           /* 8000 */
    double max_ashift;            /* 15 */
    double max_moment_nsig2;      /* 25 */
    double guess_sig;             /* 5 */
    int max_mom2_iter;            /* 400 */
    int reserved;
} imcom_star_params;
int imcom_star_sizes(int nstar, int w, int h, int is_f64, long *out);
int imcom_star_moments(imcom_ctx *ctx, const void *frame, int is_f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h,
                       const imcom_star_params *par, double forced_scale, double *out, int memspace);
int imcom_star_window_stats(imcom_ctx *ctx, const void *map, int kind, long rows, long cols, long pitch, const short *table, const int *xi, const int *yi, int nstar,
                            int bd2, double *out, int memspace);
int imcom_star_cuts(imcom_ctx *ctx, const void *frame, int is_f64, long rows, long cols, long pitch, const int *ox, const int *oy, int nstar, int w, int h, float *out,
                    int memspace);

/* World coordinate systems (reference src/pyimcom/wcsutil.py:419-634, PyIMCOM_WCS: a FITS TAN-SIP header, or for gwcs input -- type
 * "ASTROPY+" -- a fitted TAN-SIP plus a bilinear error map; src/pyimcom/utils/compareutils.py:63-106, map_sca2sca; wcsutil.py:688-788,
 * get_pix_area).  The arithmetic is that of the published definitions (FITS WCS papers I / II, the SIP convention), evaluated per point in
 * float64; it has not been compared with astropy / wcslib.  One owner thread a point, integer counts only: the same bits for every run.
 * A WCS is a caller-packed descriptor `wcs` of 130 doubles in HOST memory, whatever `memspace` says:
 *   [0] projection: 0 TAN (with or without SIP), 1 STG      [1] CRPIX1  [2] CRPIX2      [3..6] CD1_1 CD1_2 CD2_1 CD2_2, degrees a pixel
 *   [7..15] R, row-major: native unit vector = R (celestial unit vector) -- Paper II eq. (2) with the native pole at CRVAL and
 *           phi_p = LONPOLE, formed by the caller once and rounded once
 *   [16] A_ORDER  [17] B_ORDER (0: no polynomial; at most 9)      [18] niter, the fixed-point steps of the inverse's error map (0 .. 16)
 *   [19] 0      [20 + i(p, q)] A_p_q   [75 + i(p, q)] B_p_q with i(p, q) = 10 p - p (p - 1) / 2 + q, p + q <= 9
 * Anything else -- another projection, PV terms, look-up distortions, more than two axes -- cannot be packed; a projection code other than
 * 0 / 1 or an order above 9 is IMCOM_ERR_UNSUPPORTED.  The optional error table (tab NULL: none) is passed beside it: tab [2][n2][n2] of
 * float32 (tab_f64 0) or float64 (1), plane 0 the x offset and plane 1 the y offset, axes (y, x), n2 = N + 2 nodes an axis at tab_lo, 0, 1,
 * .., N - 1, tab_hi -- the padded grid and values of LocWCS.err_interp (wcsutil.py:364-413); bilinear inside, linear beyond both ends,
 * accumulated in float64.  Each point takes its OWN correction (the reference's pos[::-1, :] of lines 516 / 589 takes another point's).
 * origin: 0 or 1, the index of the first pixel.  Points written NaN (and counted): the far hemisphere of TAN, the antipode of STG, input
 * that is not finite, a SIP inverse whose Newton iteration (analytic Jacobian, from the linear solution) has not stopped after 12 steps; it
 * stops at steps below 2^-40 pixel in both components, or -- more than 4096 pixels from CRPIX, where an ulp of the coordinate exceeds
 * 2^-40 pixel -- below 2^-52 of the coordinate.
 *   imcom_wcs_sizes      no context: out[4] = {workspace bytes of a list or map call with device arrays, of imcom_wcs_pix_area with device
 *                        arrays for a W x H frame, doubles of a descriptor, the largest SIP order}.
 *   imcom_wcs_pix2world  524-560: pix [n][2] -> world [n][2] = (ra in [0, 360), dec) in degrees; with a table world(pos + dp(pos)).
 *                        *nbad (may be NULL; not NULL: the call waits for it): points written NaN.
 *   imcom_wcs_world2pix  598-634: world [n][2] -> pix [n][2]; with a table pos2 = inverse(world), then niter times pos1 = pos2 - dp(pos1)
 *                        from pos1 = pos2 (583-591).
 *   imcom_wcs_pix2pix    compareutils.py:94-106: pixels of `from` -> pixels of `to` through the unit vector alone (no ra, no dec, no
 *                        trigonometric function).  The points are a list points [n][2], or (points NULL) the grid {lo_x, step_x, count_x,
 *                        lo_y, step_y, count_y} (six doubles in HOST memory, whatever `memspace` says), row-major over (y, x):
 *                        map_sca2sca's meshgrid with pad and subsamp.  At most 2^40 points a call; nside and pad finite.  x, y [n] (both or
 *                        neither): float64, or float32 with out_f32.  is_in_ref (uint8 [n], may be NULL): lines 103-105 with `nside` and
 *                        `pad`, strict in x and not in y, from the float64 positions before any cast.  counts (HOST long [2], may be
 *                        NULL; not NULL: the call waits): {points in the reference, points written NaN}.  With x, y, is_in_ref all NULL
 *                        only the counts are formed (get_overlap_matrix, 161-167).
 *   imcom_wcs_pix_area   wcsutil.py:729-786 in two launches: ra, dec of the frame (xs [W], ys [H]: the two linspaces of 718-726) with the
 *                        exact extrema of ra; the host decides the turn of 740-749 (*rotated, may be NULL); then the centred differences
 *                        over op = ovsamp pad points, / 2 / pad, the determinant and cos(dec): area [H - 2 op][W - 2 op], square degrees.
 *   imcom_wcs_effective_gain   Sca_img's effective gain (imdestripe.py:281-297 with get_coordinates(pad=2.0), 451-474): ra, dec in degrees of
 *                        the pixels -1 .. nside on both axes, the four centred differences / 2, their determinant and 1 / (|det| cos(dec)),
 *                        with no turn away from the prime meridian (the reference has none here).  gain [nside][nside], float64 or (out_f32)
 *                        float32.  Kept from 292-293: the determinants come back transposed, so gain[i][j] has the determinant of pixel
 *                        (row j, column i) and the cosine of pixel (row i, column j). */
int imcom_wcs_sizes(long n, int W, int H, long *out);
int imcom_wcs_pix2world(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *pix, long n, int origin,
                        double *world, long *nbad, int memspace);
int imcom_wcs_world2pix(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *world, long n, int origin,
                        double *pix, long *nbad, int memspace);
int imcom_wcs_pix2pix(imcom_ctx *ctx, const double *from, const void *ftab, int ftab_f64, int ftab_n2, double ftab_lo, double ftab_hi, const double *to, const void *ttab,
                      int ttab_f64, int ttab_n2, double ttab_lo, double ttab_hi, const double *points, const double *grid, long n, int origin, double nside, double pad,
                      void *x, void *y, int out_f32, unsigned char *is_in_ref, long *counts, int memspace);
int imcom_wcs_pix_area(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, const double *xs, int W, const double *ys,
                       int H, int op, double pad, double *area, int *rotated, int memspace);
int imcom_wcs_effective_gain(imcom_ctx *ctx, const double *wcs, const void *tab, int tab_f64, int tab_n2, double tab_lo, double tab_hi, int nside, void *gain,
                             int out_f32, int memspace);

/* ---- a block's input-stamp pool from two WCSs (seam 17): InImage.partition_pixels coadd.py:329-358, InImage.extract_layers 394-404 and
 * InStamp.__init__ 688-707, between the device WCS above and imcom_select_pixels.  Arrays marked (device) are device pointers, those marked
 * (host) host pointers; there is no memspace argument.  pyimcom_amd/inpool.py is the caller.
 *
 *   imcom_partition_wcs  coadd.py:329-358 with the positions formed where they are used.  `from` (the input image) and `to` (the block) with
 *                        their optional error tables are the arguments of imcom_wcs_pix2pix (descriptors (host), tables (device)).
 *                        sp_arr [sp_res + 1] u16 (host) is the sparse axis of line 201 -- np.linspace(..., dtype=np.uint16) truncates, so the
 *                        cells are not of one size -- and relevant [sp_res][sp_res] u8 (host) the relevant_matrix of 211-233.  The visited
 *                        pixels are those of the relevant cells row-major, row-major inside a cell; cell (j, i) spans the columns
 *                        sp_arr[i] .. sp_arr[i + 1] and the rows sp_arr[j] .. sp_arr[j + 1] (335-337).  A visit index is decoded to its pixel
 *                        on the device from a prefix sum over the relevant cells; the pixel's position is that of imcom_wcs_pix2pix for the
 *                        integer pixel, origin 0, bit for bit (338).  mask [nside][nside] u8 (device; 0 = masked; NULL = none) is the FRAME
 *                        mask of 345; use_instamps, nst, n2, pix_lower, pix_upper, npixmax and the five outputs (device, zeroed by the caller)
 *                        are those of imcom_partition_pixels, and a pixel is kept or dropped exactly as there (343-351; a NaN position is
 *                        dropped).  *nvisited (may be NULL): the visited pixels.  IMCOM_ERR_ARG if a stamp would receive more than npixmax.
 *   imcom_extract_layers 394-404: data [n_inframe][nstamps][max_count] f32 with data[f][s][k] = indata[f][y_idx[s][k]][x_idx[s][k]] for
 *                        k < pix_count[s] and zero beyond, from indata [n_inframe][nside][nside] f32 and the y_idx, x_idx [nstamps][npixmax]
 *                        u16, pix_count [nstamps] u32 of the partition (all device); every element of data is written.
 *   imcom_pool_assemble  688-707 for all stamps at once: image m of n_img (in list order) has its pixels in x_src[m], y_src[m] (f64) and
 *                        data_src[m] (f32, n_inframe planes frame_stride[m] elements apart) -- pointer lists (host) of device arrays --, the
 *                        count[m][s] pixels of stamp s from element s xy_pitch[m] (x, y) and s data_pitch[m] (a plane of data); a pitch of 0
 *                        says that the image's list is compact, stamp after stamp.  xy_pitch, data_pitch, frame_stride [n_img] long, expo_of
 *                        [n_img] int and count [n_img][nstamps] u32 are host arrays; the entry forms the prefix sums.  Written (device): the
 *                        pool of imcom_select_pixels -- x, y [npool] f64, data [n_inframe][npool] f32, expo [npool] i32 (= expo_of[m]; NULL:
 *                        not wanted) -- with the stamps row-major, inside a stamp the images in list order and an image's pixels in its own
 *                        order (698-707), and inst_off [nstamps + 1] i64.  npool must be the sum of count.  A segmented copy; no sort. */
int imcom_partition_wcs(imcom_ctx *ctx, const double *from, const void *ftab, int ftab_f64, int ftab_n2, double ftab_lo, double ftab_hi, const double *to,
                        const void *ttab, int ttab_f64, int ttab_n2, double ttab_lo, double ttab_hi, const unsigned short *sp_arr, const unsigned char *relevant,
                        int sp_res, int nside, const unsigned char *mask, const unsigned char *use_instamps, int nst, int n2, double pix_lower, double pix_upper,
                        int npixmax, unsigned short *y_idx, unsigned short *x_idx, double *y_val, double *x_val, unsigned int *pix_count, long *nvisited);
int imcom_extract_layers(imcom_ctx *ctx, const float *indata, int n_inframe, int nside, const unsigned short *y_idx, const unsigned short *x_idx,
                         const unsigned int *pix_count, int nstamps, int npixmax, int max_count, float *data);
int imcom_pool_assemble(imcom_ctx *ctx, int n_img, int nstamps, int n_inframe, const void *const *x_src, const void *const *y_src, const void *const *data_src,
                        const long *xy_pitch, const long *data_pitch, const long *frame_stride, const int *expo_of, const unsigned int *count, long npool, double *x,
                        double *y, float *data, int *expo, long *inst_off);

/* ---- The input-layer cube (seam 23): reference src/pyimcom/layer.py:1199-1527, get_all_data, fills inimage.indata [n_inframe][nside][nside]
 * float32 plane by plane.  imcom_layer_place writes every plane that no generator writes: the science frame minus its sky (1261, 1264),
 * truth with its flip and rescale (1284-1295), labnoise with the literal crop [4:4092, 4:4092] and its flip (1322-1335), skyerr (1344), a
 * saved noise slice (1484), and the float64 images of the white-noise (1304) and star-grid (1351) seams on their way into the cube.
 *
 *   dst[y][x] = post(op(src[y0 + sy][x0 + sx])),  (sy, sx) = (y, x), (y, nside - 1 - x) for flip 1 (`[:, ::-1]`), (nside - 1 - y, x) for
 *               flip 2 (`[::-1, :]`); src [src_ny][src_nx] of src_type 0 float32, 1 float64, 2 int16, 3 uint16, 4 int32, 5 uint8; with
 *               src_swapped = 1 its elements are in the other byte order than the machine's (a FITS image as the file holds it) and
 *               are swapped as they are read.
 *   op          0: the value as it is; 1: value - sub, as numpy >= 2 forms `data - float(sky)`: float32 - float32(sub) in float32 for a
 *               float32 source, else the exact double of the value minus sub in double.
 *   the result  rounded to float32 to nearest even (a float32 source is not rounded again), then with post_scale_flag = 1 multiplied by
 *               float32(scale) in float32 (`plane *= rescale`, 1295).  NaN stays NaN, infinities pass, -0.0 keeps its sign.
 *
 * src and dst follow `memspace` (host: staged through the workspace, the call waits; device: one launch on the context's stream, pointers
 * aligned to their elements).  IMCOM_ERR_ARG, before anything is queued, for a type, flip, op or flag outside its range, a side outside
 * 0 .. 65536 and a window that leaves the source (y0, x0 < 0, y0 + nside > src_ny, x0 + nside > src_nx); nside = 0 is a no-op. */
int imcom_layer_place(imcom_ctx *ctx, const void *src, int src_type, int src_swapped, int src_ny, int src_nx, int y0, int x0, int flip, int op, double sub,
                      int post_scale_flag, double scale, float *dst, int nside, int memspace);

/* ---- HEALPix star grids (seam 18): the pixels of the RING scheme (Gorski et al. 2005, ApJ 622, 759; nside = 2^res, res 0 .. 29, int64
 * indices) inside a circle on the sky, their centres, and those centres through a WCS.  healpy is not needed; the arithmetic is that of the
 * paper (section 4.1, eqs. 2-9, and the inverse) in float64 and has not been compared with healpy.  NEST order is not served.
 *
 *   imcom_healpix_pix2ang  healpy.pix2ang(2**res, ipix, nest=False, lonlat=lonlat) (analysis.py:964, truthcats.py:203, starcube_nonoise.py,
 *                          dynrange.py): ipix [n] -> a, b [n] = (theta, phi) in radians, or with lonlat (lon, lat) = (degrees(phi),
 *                          90 - degrees(theta)).  A pixel outside 0 .. 12 * 4^res - 1 is IMCOM_ERR_ARG (its outputs are NaN).
 *   imcom_healpix_ang2pix  healpy.ang2pix(2**res, a, b, nest=False, lonlat=lonlat) (layer.py:724-725): the pixel that holds each point; phi is
 *                          reduced into [0, 2 pi).  An angle that is not finite, or a colatitude outside [0, pi], is IMCOM_ERR_ARG (its pixel
 *                          is -1).
 *   imcom_healpix_cap      GridInject.make_sph_grid and generate_star_grid (layer.py:690-789), and healpy.ang2vec + query_disc + pix2ang +
 *                          all_world2pix + the box selection of analysis.py:957-978, starcube_nonoise.py:145-175, dynrange.py:167-191 and
 *                          truthcats.py:190-241.  Centre (ra, dec) and radius in radians.  mode 0: the reference's contiguous pixel range
 *                          pmin .. pmax of layer.py:721-725 (a cap that holds a pole loses the pixels of the polar ring beyond it); mode 1:
 *                          the full disc, what query_disc(inclusive=False) returns.  A pixel belongs when mu = sin(dec_p) sin(dec) +
 *                          cos(dec_p) cos(dec) cos(ra - phi_p) >= cos(radius) in float64 (layer.py:732-733).  Outputs, each [capacity] and
 *                          each NULL or not, ascending in the pixel: ipix; ra_pix, dec_pix in radians (phi and pi / 2 - theta); ra_deg,
 *                          dec_deg in degrees -- lonlat 0: rad / (pi / 180) as layer.py:787-789 forms them, lonlat 1: healpy's lonlat values;
 *                          with a WCS (`wcs` .. `origin`: the arguments of imcom_wcs_world2pix, NULL: none) x, y of (ra_deg, dec_deg), the bits
 *                          imcom_wcs_world2pix gives; pa, the position angle of truthcats.py:229-241 in degrees in [0, 360).  box_n > 0 keeps
 *                          only the pixels with box_bdpad <= rint(x) < box_n - box_bdpad and the same in y (analysis.py:967-973; a rint that
 *                          does not fit int16 is outside).  *count (HOST, may be NULL): the pixels selected.  With every output NULL only
 *                          the count is formed; otherwise capacity must equal the count (IMCOM_ERR_ARG if not): count, allocate, fill.
 *                          At most 2^22 rings a call.  No atomics: the same bits for every run. */
int imcom_healpix_pix2ang(imcom_ctx *ctx, int res, const long *ipix, long n, int lonlat, double *a, double *b, int memspace);
int imcom_healpix_ang2pix(imcom_ctx *ctx, int res, const double *a, const double *b, long n, int lonlat, long *ipix, int memspace);
int imcom_healpix_cap(imcom_ctx *ctx, int res, double ra, double dec, double radius, int mode, int lonlat, const double *wcs, const void *tab, int tab_f64, int tab_n2,
                      double tab_lo, double tab_hi, int origin, int box_n, int box_bdpad, long capacity, long *ipix, double *ra_pix, double *dec_pix, double *ra_deg,
                      double *dec_deg, double *x, double *y, double *pa, long *count, int memspace);

/* ---- the metadetection mosaic (seam 19): what MetaMosaic (src/pyimcom/meta/distortimage.py) does to its arrays before and between the
 * calls of imcom_ginterp_resample.  Every pointer is DEVICE memory; there is no memspace argument and nothing waits for the device.  The
 * mosaic is in_image [nlayer][ns][ns] (float32 or float64), in_fidelity and in_noise [ns][ns] float32 (dB) and in_mask [ns][ns] u8; ns <=
 * 32768; in_image, in_fidelity and in_noise 16-byte aligned, the masks 4-byte aligned.  pyimcom_amd/metamosaic.py is the caller.
 *
 *   imcom_mosaic_paste     distortimage.py:191-207 for one block file, one launch: the window rows symin .. symax - 1, columns sxmin ..
 *                          sxmax - 1 of the file's planes (by x bx pixels) go to the rows cy + symin .., columns cx + sxmin .. of the mosaic
 *                          (146-170 give the six numbers; a window that leaves the file or the mosaic is IMCOM_ERR_ARG).  primary: nlayer
 *                          planes layer_stride elements apart, rows row_stride elements apart, float32 or (prim_f64) float64, copied bit for
 *                          bit.  fid, sig: the coded FIDELITY and SIGMA planes, rows fid_stride / sig_stride elements apart, of type 0 = uint8,
 *                          1 = uint16, 2 = int16.  in_fidelity = float(code) * (float)fid_bels / (float)(-0.1) and in_noise = float(code) *
 *                          (float)sig_bels / (float)0.1, each two correctly rounded float32 operations as numpy's 197-207 are (bels: what
 *                          HDU_to_bels gave; NaN allowed).  in_mask = (in_fidelity == 0) on the window (210).  16-byte accesses along a row
 *                          where source and destination agree in their offset within 16 bytes, element by element elsewhere.
 *   imcom_mosaic_mask_cut  223-280 and 499-503: mask [n] |= map [n] < cut (mode 1), |= map > cut (mode 2), nothing (mode 0; map may be NULL),
 *                          and |= extra [n] != 0 (extra NULL: none).  The float32 map value and cut are compared as doubles; NaN is false.
 *   imcom_mosaic_caps      340-352: n circles at the pixel positions (x, y) with the radii r (float64 [n], pixels).  Circle j sets the pixels
 *                          (ix, iy) of its box xmin = max(floor(x - r), 0) .. xmax = min(ceil(x + r) + 1, ns) (341-344; float64, clamped to
 *                          [0, ns] before the conversion to an integer; the same in y) with hypot(ix - x, iy - y) < r.  A position or radius
 *                          that is not finite sets nothing.  Three launches: boxes, their prefix sum, and the pixels of all boxes as one
 *                          flat index space in chunks of 4096 strided over the grid -- one large circle is spread over the whole device and
 *                          small ones share a wave.  The only writes are byte stores of 1: the result depends neither on the order of the
 *                          objects nor on the launch.  Workspace: 24 bytes an object. */
int imcom_mosaic_paste(imcom_ctx *ctx, const void *primary, int prim_f64, long layer_stride, long row_stride, int nlayer, int by, int bx, const void *fid,
                       int fid_type, long fid_stride, double fid_bels, const void *sig, int sig_type, long sig_stride, double sig_bels, int symin, int symax,
                       int sxmin, int sxmax, int cy, int cx, int ns, void *in_image, float *in_fidelity, float *in_noise, unsigned char *in_mask);
int imcom_mosaic_mask_cut(imcom_ctx *ctx, unsigned char *mask, const float *map, long n, double cut, int mode, const unsigned char *extra);
int imcom_mosaic_caps(imcom_ctx *ctx, const double *x, const double *y, const double *r, long n, int ns, unsigned char *mask);

/* Padding stamps shared between neighbouring blocks (reference src/pyimcom/analysis.py:394-537, OutImage._update_hdu_data; the loop of
 * Mosaic.share_padding_stamps, 1429-1467, is the caller's): with pad_sides = "auto" a block coadds no padding stamps towards a neighbour,
 * and "my" strip on that side is filled from the neighbour's interior afterwards.  direction: 0 left, 1 right (a range of columns),
 * 2 bottom, 3 top (a range of rows).  With width = postage_pad * n2 and fk = fade_kernel my strip is 0 .. width + fk - 1 (left, bottom) or
 * NsideP - width - fk .. NsideP - 1 (right, top), and the neighbour's is NsideP - 2 width .. NsideP - width + fk - 1 or width - fk ..
 * 2 width - 1 (435-446).  Every entry refuses direction outside 0 .. 3, width < fk and 2 width > NsideP (IMCOM_ERR_ARG), reads the
 * neighbour, writes only my strip, and refuses mine == theirs: the two blocks are distinct allocations.  All pointers are device memory
 * except the two small tables, which are host memory and go through the pinned ring.
 *
 *   imcom_padshare_layers   435-450, PRIMARY: mine[strip] = mine[strip] * add_mode + theirs[strip] on nplanes (= n_out * nlayer) float32
 *                           planes, rows `row` and planes `plane` elements apart on either side (a view of BlockMaps.out_map cropped by
 *                           fk is updated in place).  The product by the bool is formed in float32 as numpy forms it: in replace mode
 *                           (add_mode = 0) -0.0 of mine gives +0.0 and a value of mine that is not finite gives NaN.  One launch.
 *   imcom_padshare_weights  453-488, INWEIGHT [n_out][n_mine | n_theirs][n1P][n1P] float32: for each of the npairs rows (my_idx, ur_idx) of
 *                           pairs_host -- the first occurrences of an (obsid, sca) that both INDATA tables hold, 468-470 -- the strip of
 *                           `pad` stamps is copied (never added; the strips are those above with n1P, pad, 0 for NsideP, width, fk).  A
 *                           my_idx may appear once.  One launch; npairs = 0 is a no-op.
 *   imcom_padshare_maps     498-537, the quality maps, all nmaps of them in one launch.  Both codes of a strip pixel are decoded as
 *                           get_output_map decodes them (377-387): float32(pow(10.0, code / decode_coef)) with decode_coef the double
 *                           1.0 / HDU_to_bels(hdu), and 0 for the code floor_code (IMCOM_PADSHARE_NO_FLOOR: for none -- whether line 387
 *                           zeroes the floor depends on the numpy beside the reference, and the caller decides).  In add mode both are
 *                           tapered as OutStamp.trapezoid tapers them (coadd.py:1269-1282, pad widths of 504-526; one product in
 *                           double, rounded to float32).  mine * add_mode + theirs in float32 goes to sums ([n_out][strip], the strip
 *                           row-major as numpy slices it; NULL in production) and, encoded as Block.compress_map encodes
 *                           (coadd.py:2123-2130, see imcom_compress_map_f32) with the integer encode_coef, into my strip.
 *                           Codes: [n_out][NsideP][NsideP] int16 or (is_unsigned) uint16. */
#define IMCOM_PADSHARE_NO_FLOOR (1 << 20)
typedef struct imcom_padshare_map {
    void *mine;          /* my codes, updated in place */
    const void *theirs;  /* the neighbour's codes */
    double decode_coef;  /* 1.0 / HDU_to_bels */
    float *sums;         /* NULL, or where the float32 sums before the encode go */
    int floor_code;      /* the code that decodes to 0, or IMCOM_PADSHARE_NO_FLOOR */
    int encode_coef;     /* int(comment.partition("*")[0]), analysis.py:530 */
    int is_unsigned;
    int reserved;
} imcom_padshare_map;
int imcom_padshare_layers(imcom_ctx *ctx, int direction, int add_mode, int nside_p, int width, int fk, long nplanes, float *mine, long mine_row,
                          long mine_plane, const float *theirs, long theirs_row, long theirs_plane);
int imcom_padshare_weights(imcom_ctx *ctx, int direction, int n_out, int n1P, int pad, int npairs, const int *pairs_host, float *mine, int n_mine,
                           const float *theirs, int n_theirs);
int imcom_padshare_maps(imcom_ctx *ctx, int direction, int add_mode, int nside_p, int width, int fk, int n_out, int nmaps,
                        const imcom_padshare_map *maps_host);

#ifdef __cplusplus
}
#endif
#endif /* IMCOM_HIP_H */
