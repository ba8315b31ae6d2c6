// chol_solve.hip -- the host-side orchestration of the batched blocked Cholesky solve (no kernel and no launch of its own: the launches are
// gemm_f64.hip's, la_kernels.hip's, chol_diag.hip's and lmin_skinny.hip's): the workspace plans, the repair of a failed factorisation with
// the smallest eigenvalue (lambda_min_subspace), chol_core, and the C-ABI entries imcom_solve_chol*, which end the file.
#include <chrono>
#include <cmath>
#include <functional>

#include "common.h"
#include "launchers.h"

namespace imcom {

// -------------------------------------------------------------------------------------------------
// Batched blocked Cholesky solve on padded, device-resident operands.
//   A  [batch][Np][Np]   identity-padded, never modified
//   Bt [batch][Np][mp]   input-pixel-major -B/2, zero padded
// Produces Tt (float32 [batch][Np][mp]) and the per-pixel maps.
constexpr int REPAIR_GROUP = 32;  // failed stamps whose smallest eigenvalues are computed in one batch of the eigensolver (repair path, small matrices / fallback)
constexpr int CHOL_MAXNV = 8;  // kappa nodes of the multi-kappa Cholesky kernel (launch_multi's MAXNV; 3 nv diagonal increments <= MAX_INC)
static_assert(3 * CHOL_MAXNV <= MAX_INC_HOST, "diagonal increments of the repair sequence");
constexpr int LMIN_P = NB;        // vectors the workspace plan of the smallest-eigenvalue iteration is sized for (see lmin_ws_bytes)
constexpr int LMIN_MIN_N = 1024;  // smaller matrices go through the eigensolver itself (cheap there; the block needs n >> LMIN_SKINNY_P)

// Split-K for small batches: with fewer than ~256 tiles per launch (the kernel-class seam hands over one stamp: 18) the K
// loop of every tile is dealt to up to 8 workgroups, so that a launch has ~512 of them (gemm_f64.hip).
static int splitk_parts(int batch, int tiles)
{
    const long wgs = (long)batch * tiles;
    if (wgs >= 256) return 1;
    return (int)std::min<long>(8, std::max<long>(1, 512 / std::max<long>(wgs, 1)));
}

static size_t splitk_bytes(int batch, int Np, int mp)
{
    const int tiles = std::max(Np, mp) / NB;
    return splitk_parts(batch, std::min(Np, mp) / NB) > 1 ? (size_t)batch * tiles * 8 * NB * NB * 8 + 256 : 0;
}

// Multi-kappa on a small batch: the nv factorisations and solves of a stamp are independent, so they are run as ONE pass over
// nv x batch "stamps" (node-major: exactly the layout of Y) instead of nv passes that each fill a fraction of the chip.
static int nodes_per_pass(int batch, int mp, int nv)
{
    return (nv > 1 && (long)batch * nv * (mp / NB) <= 1024) ? nv : 1;
}

static bool lmin_subspace_enabled()
{
    return !env_is("IMCOM_LMIN", "eigh");  // (cross-check: the eigensolver for every repair)
}

// workspace of lambda_min_subspace on top of the factorisation's own L / Dinv / dshift.  The plan is still the one of the 128-vector
// form the iteration had before its blocks of 16 vectors: it fixes the pass sizes of the callers that plan with it (and with them the
// timing), so it stays as it is until a change of its own, measured, shrinks it to what the 16-vector form takes.
static size_t lmin_ws_bytes(int batch, int Np)
{
    if (!lmin_subspace_enabled() || Np < LMIN_MIN_N) return 0;
    WsPlan p;
    for (int q = 0; q < 3; q++) p.add((size_t)batch * Np * LMIN_P * 8);      // X, Y, Z = A X
    for (int q = 0; q < 4; q++) p.add((size_t)batch * LMIN_P * LMIN_P * 8);  // G, its inverse Cholesky factor, H = X^T A X, H's eigenvectors
    p.add((size_t)batch * LMIN_P * 8);                                       // eigenvalues of H
    p.add((size_t)batch * LMIN_RESID_GROUPS * 2 * 8);                        // residuals of the two lowest Ritz pairs, by row group
    p.add((size_t)batch * 8 * NB * NB * 8);                                  // split-K partial products of the 128-column solves
    p.add((size_t)batch * 8);                                                // largest diagonal entry
    for (int q = 0; q < 4; q++) p.add((size_t)batch * 4);                    // want, ones, flags of the Gram factorisations, masked nblk
    p.add(eigh_ws_bytes(batch, LMIN_P, true));
    return p.total + 8192;
}

static size_t chol_core_bytes(int batch, int Np, int m, int mp, int nv)
{
    WsPlan p;
    const size_t nb = Np / NB, eb = (size_t)batch * nodes_per_pass(batch, mp, nv);
    p.add(eb * Np * Np * 8);                     // L
    p.add(eb * nb * NB * NB * 8);                // Dinv
    p.add((size_t)nv * batch * Np * mp * 8);     // Y / X per node
    p.add(eb * Np * 8);                          // dshift
    p.add(eb * 4 * 3 + (size_t)batch * 4 * nv);  // n, nblk, ninc, fail[nv]
    p.add((size_t)batch * 4 * 4);                // attempt masks: stamps to factor, their block counts, block counts of the solves, solved flags
    p.add(eb * MAX_INC_HOST * 8);                // inc
    p.add((size_t)batch * 8 * 2);                // kap, C
    p.add((size_t)nv * 8);                       // kappaC
    if (nv > 1) {
        p.add((size_t)batch * m * nv * 8);       // Dp
        p.add((size_t)batch * m * nv * nv * 8);  // Npq
        p.add((size_t)batch * m * nv * 8);       // W
    }
    // repair path (lakernel.py:262-279): the smallest eigenvalue of every failed stamp's A -- the subspace iteration on the stamps in
    // place (lambda_min_subspace), the eigensolver on up to REPAIR_GROUP gathered copies for small matrices and as its fallback
    const int rg = std::min(batch, REPAIR_GROUP);
    p.add(std::max(eigh_ws_bytes(rg, Np, false) + (size_t)rg * Np * Np * 8 + (size_t)rg * Np * 8 + 4096, lmin_ws_bytes(batch, Np)));
    p.add(splitk_bytes((int)eb, Np, mp));
    if (nv == 1) p.add((size_t)batch * 2 * nb * mp * 8 * 2);  // per-block-row column sums of Y^2 and X^2
    return p.total + 4096;
}

// smallest eigenvalues of the matrices A[idx[q]] (leading n x n of the padded ones), computed on the device: the stamps are
// gathered into one batch of the eigensolver (eigenvalues only).  (One call per failed stamp, as the first version did, made a
// batch in which every factorisation fails -- PSFs cut too tight -- take 0.3 s per stamp.)
static int lambda_min_group(imcom_ctx *ctx, const double *A, const int *n_host, int Np, const int *idx, int count, double *w0)
{
    const size_t mark = ctx->ws_used;
    const size_t mat = (size_t)Np * Np;
    double *G = (double *)ws_take(ctx, (size_t)count * mat * 8);
    double *lam = (double *)ws_take(ctx, (size_t)count * Np * 8);
    if (!G || !lam) return ws_short("repair");
    std::vector<int> ng(count);
    for (int q = 0; q < count; q++) {
        ng[q] = n_host[idx[q]];
        IMCOM_HIP_CHECK(hipMemcpyAsync(G + (size_t)q * mat, A + (size_t)idx[q] * mat, mat * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    int rc = eigh_device(ctx, count, ng.data(), Np, G, Np, (long)mat, lam, Np, nullptr, Np, (long)mat, nullptr);  // eigenvalues only
    if (rc == IMCOM_OK) {
        hipError_t e = hipMemcpy2DAsync(w0, 8, lam, (size_t)Np * 8, 8, count, hipMemcpyDeviceToHost, ctx->stream);  // lam[q][0]
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { set_error("repair: %s", hipGetErrorString(e)); rc = IMCOM_ERR_HIP; }
    }
    ctx->ws_used = mark;
    return rc;
}

// The smallest eigenvalue of the stamps `idx` WITHOUT an eigendecomposition (the reference's repair needs w[0] of eigh(A) and nothing
// else, lakernel.py:266-268).  A production stamp (configs/paper4_configs/H158_Chol_benchmark.json: N ~ 6.2k pixels) has thousands of
// eigenvalues within 1e-5 |A| of zero and a smallest one of either sign; the tridiagonalisation of a 6.2k matrix costs 4 N^3 / 3 flops at
// memory speed (95 ms per stamp), the kernels this library is fast at are the blocked Cholesky and the triangular solves.  So:
//   1. a shift sigma with A + sigma I positive definite (trial factorisations, sigma x 8 per failure; the first trial is 4 x the
//      increment the failed factorisation had);
//   2. subspace iteration with the inverse, X <- orth((A + sigma I)^-1 X), on a block of 16 vectors (lmin_skinny.hip: CholQR twice
//      per step), then Rayleigh-Ritz with A ITSELF: theta = lambda_min(X^T A X) >= lambda_min(A), accurate to eps |A| once the block has
//      converged -- the accuracy class of LAPACK's own w[0] -- with the residuals of the two lowest Ritz pairs as the error bound;
//   3. re-factor at sigma' = |theta| (1 + eta) just above the estimate (eta from that bound; a sigma' that is not above
//      |lambda_min| makes the factorisation fail: eta x 8), where the block converges by 1e-3 and more per step; stop when the bound is
//      below 1e-11 |theta| (or two successive Rayleigh-Ritz values agree to that).
// Everything runs on the stamps in place (L, Dinv, dshift of the caller's factorisation; stamps that are not wanted have no blocks in
// these launches).  factor(shift, mask, fail): L L^T = A + shift[s] I for the stamps of mask, fail[s] != 0 where that is not positive
// definite; solve(mask, X, Y, part): Y = (L L^T)^-1 X on LMIN_SKINNY_P columns (part: scratch of the few-stamp form).  ok[s] = 0: no
// answer (the caller takes the eigensolver).
static int lambda_min_subspace(imcom_ctx *ctx, int batch, const int *n_host, const int *n_dev, int Np, const double *A, const std::vector<int> &idx,
                               const std::vector<double> &inc_failed, double hint, const std::vector<char> &may_decide, std::vector<char> &decided,
                               const std::function<int(const std::vector<double> &, const std::vector<char> &, std::vector<int> &)> &factor,
                               const std::function<int(const std::vector<char> &, const double *, double *, double *)> &solve,
                               std::vector<double> &w0, std::vector<char> &ok)
{
    const size_t mark = ctx->ws_used;
    // Blocks of 16 vectors instead of 128 (lmin_skinny.hip): with a shift a few per cent above |lambda_min| the block's width hardly
    // matters for the convergence (7-9 steps against 5-7 on a production stamp), and a 16-column sweep is one pass over the factor at
    // HBM speed instead of a 128-column product on the matrix pipe.  Two forms of the sweeps: a pass of more than 128 stamps runs a
    // workgroup per stamp; fewer stamps (the kernel-class seam hands over one or four; a block's short last pass) two short launches
    // per block row with the sums dealt to many workgroups (on a pass of 168 stamps the two are within 2 % of each other: 1960
    // launches per pass against 10).
    constexpr int P = LMIN_SKINNY_P;
    const size_t blk = (size_t)batch * Np * P * 8;
    double *X = (double *)ws_take(ctx, blk), *Y = (double *)ws_take(ctx, blk), *Z = (double *)ws_take(ctx, blk);
    double *lam = (double *)ws_take(ctx, (size_t)batch * P * 8);
    double *rpart = (double *)ws_take(ctx, (size_t)batch * LMIN_RESID_GROUPS * 2 * 8);
    double *part = (double *)ws_take(ctx, (size_t)batch * 8 * NB * NB * 8);
    double *dmax_d = (double *)ws_take(ctx, (size_t)batch * 8);
    int *want_d = (int *)ws_take(ctx, (size_t)batch * 4), *gfail_d = (int *)ws_take(ctx, (size_t)batch * 4);
    int *nbrun_d = (int *)ws_take(ctx, (size_t)batch * 4);  // 128-blocks of the stamps a round runs (0: not in it)
    if (!X || !Y || !Z || !lam || !rpart || !part || !dmax_d || !want_d || !gfail_d || !nbrun_d) return ws_short("smallest eigenvalue");
    hipStream_t st = ctx->stream;
    std::vector<char> want(batch, 0);
    std::vector<int> want_i(batch, 0);
    for (int s : idx) { want[s] = 1; want_i[s] = 1; }
    IMCOM_TRY(upload(ctx, want_d, want_i.data(), (size_t)batch));
    IMCOM_HIP_CHECK(hipMemsetAsync(gfail_d, 0, (size_t)batch * 4, st));
    IMCOM_HIP_CHECK(hipMemsetAsync(Y, 0, blk, st));
    IMCOM_HIP_CHECK(hipMemsetAsync(Z, 0, blk, st));
    IMCOM_TRY(launch_diag_max(ctx, A, Np, n_dev, dmax_d, batch));
    std::vector<double> dmax(batch, 0.0);
    IMCOM_HIP_CHECK(hipMemcpyAsync(dmax.data(), dmax_d, (size_t)batch * 8, hipMemcpyDeviceToHost, st));
    IMCOM_HIP_CHECK(hipStreamSynchronize(st));
    const bool dbg = env_is("IMCOM_LMIN_DEBUG");
    int nfac = 0, nfac_failed = 0, rounds_run = 0;
    // 1. a positive definite shift
    std::vector<double> sigma(batch, 0.0);
    std::vector<char> todo = want, act = want;
    std::vector<int> fail;
    // The caller's estimate of max |lambda_min| (imcom_ctx_set_repair_hint: what the pass before this one found -- over a production
    // block the largest |lambda_min| of a pass of 168 stamps stays within 1 % from pass to pass, the stamps of a pass within 6 % of
    // each other): the first shift is that estimate plus a margin instead of four times the failed increment, i.e. already as close as the
    // SECOND shift of a stamp that starts without one, and the iteration needs one factorisation instead of two.  An estimate that is too
    // small for a stamp costs that stamp one failed factorisation (then the shift it would have started with).
    const bool hint_off = env_is("IMCOM_LMIN_HINT", "0");
    constexpr double hint_margin = 0.05;
    std::vector<char> hinted(batch, 0);
    std::vector<double> base(batch, 0.0);
    bool any_hinted = false;
    for (int s : idx) {
        base[s] = sigma[s] = std::max(std::max(4.0 * inc_failed[s], 1e-13 * dmax[s]), 1e-300);
        if (!hint_off && hint > 0.0 && std::isfinite(hint)) { sigma[s] = hint * (1.0 + hint_margin); hinted[s] = 1; any_hinted = true; }
    }
    for (int t = 0;; t++) {
        IMCOM_TRY(factor(sigma, todo, fail));
        nfac++;
        bool any = false;
        for (int s : idx) {
            if (!todo[s]) continue;
            if (fail[s] != 0 && hinted[s]) { sigma[s] = std::max(base[s], 2.0 * sigma[s]); hinted[s] = 0; any = true; }
            else if (fail[s] != 0 && std::isfinite(sigma[s] * 8.0)) { sigma[s] *= 8.0; any = true; }
            else if (fail[s] != 0) { todo[s] = 0; act[s] = 0; }  // (not finite: not a matrix this iteration can help)
            else todo[s] = 0;
        }
        if (any) nfac_failed++;
        if (!any) break;
        if (t >= 24) {
            for (int s : idx) if (todo[s]) { todo[s] = 0; act[s] = 0; }
            break;
        }
    }
    // 2. / 3. subspace iteration, Rayleigh-Ritz with A, closer shifts
    IMCOM_TRY(launch_lmin_init(ctx, X, Np, P, n_dev, want_d, batch));
    auto orth = [&]() -> int {  // X <- orth(Y): CholQR twice (X = Y R^-1 with R^T R = Y^T Y; the second pass takes the loss of the first back)
        IMCOM_TRY(launch_skinny_orth(ctx, Y, X, Np, nbrun_d, gfail_d, batch));
        IMCOM_TRY(launch_skinny_orth(ctx, X, Y, Np, nbrun_d, gfail_d, batch));
        std::swap(X, Y);  // the orthonormal block is in the buffer pass 1 wrote
        return IMCOM_OK;
    };
    std::vector<double> theta(batch, 0.0), prev(batch, 0.0), eta(batch, 1e-3), lam01((size_t)batch * 2, 0.0), rp((size_t)batch * LMIN_RESID_GROUPS * 2, 0.0);
    std::vector<double> est(batch, 0.0), est_simple(batch, 0.0), dbg_th(batch, 0.0), dbg_r1(batch, 0.0), dbg_r2(batch, 0.0), dbg_g2(batch, 0.0), dbg_gP(batch, 0.0), lamP(batch, 0.0);
    std::vector<char> conv(batch, 0);
    std::vector<int> gfail(batch, 0);
    // Per stamp two phases.  Coarse, at the first shift: nine steps (ten at a hinted one), then a Rayleigh-Ritz step that also yields the residuals r1, r2 of the
    // two lowest Ritz pairs (theta1, y1), (theta2, y2) -- there is an eigenvalue within |r1| of theta1, and once theta1 is separated from
    // the rest, (theta2 - |r2|) - theta1 = gap > 4 |r1|, theta1 - lambda_min <= |r1|^2 / gap (Kato-Temple).  With that bound below 15 % the
    // stamp gets ONE factorisation at |theta1| (1 + eta), eta = 1.5 x the bound (a shift that is not above |lambda_min| makes the
    // factorisation fail: eta x 8 -- every such trial costs eight steps' time), where the block converges by 1e-3 and more per step:
    // fine rounds of three steps until the bound is below 1e-11 |theta1|, which the first one reaches on a production stamp
    // (configs/paper4: six coarse steps leave 2e-3, three fine ones 1e-13).  The change between two successive values of theta1 -- the
    // criterion of the first version, which cost a round of three steps and a Rayleigh-Ritz step in each phase only to confirm -- still
    // ends either phase when the residuals cannot (theta1 inside a cluster closer than its residual).
    constexpr int coarse_steps = 9;   // (16 vectors at a blind shift: six steps leave 25-40 %, nine a few per cent)
    constexpr int hinted_steps = 10;  // (at a hinted shift, see above)
    constexpr int round_steps = 3;    // steps of a fine round
    // how far the spectrum the block has NOT captured lies above lambda_min, in units of |lambda_min| (production stamps: lambda_17 is 0.4
    // of the way to zero): the step counts below are planned with it
    constexpr double bulk = 0.4;
    const int max_rounds = 14;
    std::vector<char> fine(batch, 0);
    std::vector<int> steps_wanted(batch, 0);
    std::vector<double> lastrel(batch, 1.0);
    for (int round = 0; round < max_rounds; round++) {
        std::vector<char> run(batch, 0);
        bool any = false;
        for (int s : idx) if (act[s] && !conv[s]) { run[s] = 1; any = true; }
        if (!any) break;
        int iters = round == 0 ? (any_hinted ? hinted_steps : coarse_steps) : round_steps;
        for (int s : idx) if (run[s]) iters = std::max(iters, steps_wanted[s]);  // (a stamp's first round at its closer shift: see below)
        std::fill(steps_wanted.begin(), steps_wanted.end(), 0);
        int nbrun_max = 0;
        std::vector<int> nbr(batch, 0);
        for (int s : idx) if (run[s]) { nbr[s] = (n_host[s] + NB - 1) / NB; nbrun_max = std::max(nbrun_max, nbr[s]); }
        IMCOM_TRY(upload(ctx, nbrun_d, nbr.data(), (size_t)batch));
        for (int it = 0; it < iters; it++) {
            IMCOM_TRY(solve(run, X, Y, part));
            IMCOM_TRY(orth());
        }
        // Z = A X, H = X^T Z, its eigenvalues, the residuals of the two lowest pairs
        IMCOM_TRY(launch_skinny_ax(ctx, A, X, Z, Np, nbrun_d, nbrun_max, batch));
        IMCOM_TRY(launch_skinny_rr(ctx, X, Z, Np, nbrun_d, lam, rpart, LMIN_RESID_GROUPS, batch));
        IMCOM_HIP_CHECK(hipMemcpy2DAsync(lam01.data(), 16, lam, (size_t)P * 8, 16, batch, hipMemcpyDeviceToHost, st));
        IMCOM_HIP_CHECK(hipMemcpyAsync(rp.data(), rpart, rp.size() * 8, hipMemcpyDeviceToHost, st));
        IMCOM_HIP_CHECK(hipMemcpy2DAsync(lamP.data(), 8, lam + P - 1, (size_t)P * 8, 8, batch, hipMemcpyDeviceToHost, st));
        IMCOM_HIP_CHECK(hipMemcpyAsync(gfail.data(), gfail_d, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
        IMCOM_HIP_CHECK(hipStreamSynchronize(st));
        std::vector<char> refac(batch, 0);
        bool any_refac = false;
        for (int s : idx) {
            if (!run[s]) continue;
            const double th1 = lam01[2 * (size_t)s], th2 = lam01[2 * (size_t)s + 1];
            double q1 = 0.0, q2 = 0.0;
            for (int g = 0; g < LMIN_RESID_GROUPS; g++) { q1 += rp[((size_t)s * LMIN_RESID_GROUPS + g) * 2]; q2 += rp[((size_t)s * LMIN_RESID_GROUPS + g) * 2 + 1]; }
            if (gfail[s] != 0 || !std::isfinite(th1) || !std::isfinite(q1) || !std::isfinite(q2)) { act[s] = 0; continue; }  // the block lost rank / not a number: the eigensolver's case
            const double r1 = sqrt(q1), r2 = sqrt(q2), gap = (th2 - r2) - th1, mag = std::max(fabs(th1), 1e-300);
            est_simple[s] = r1;
            if (dbg && round == 0) { dbg_th[s] = th1; dbg_r1[s] = r1; dbg_r2[s] = r2; dbg_g2[s] = th2 - th1; dbg_gP[s] = lamP[s] - th1; }
            // theta1 - lambda_min >= 0: at most |r1|, at most |r1|^2 / gap once theta1 is separated (both rigorous) -- and in fact close to
            // |r1|^2 / (theta_P - theta1), the distance to the part of the spectrum the block has NOT captured (the lowest eigenvalues of a
            // stamp's A come in near-degenerate pairs, so the rigorous gap is tiny while theta1's error is governed by the bulk near zero:
            // on 128 paper4 stamps the error was 1.03 ... 1.28 x that quotient after six coarse steps and after three fine ones)
            const double span = lamP[s] - th1;
            est[s] = gap > 4.0 * r1 ? r1 * r1 / gap : r1;
            if (span > 4.0 * r1) est[s] = std::min(est[s], 3.0 * r1 * r1 / span);
            prev[s] = theta[s];
            theta[s] = th1;
            const double rel = round == 0 ? 1.0 : fabs(theta[s] - prev[s]) / mag;
            const double bound = est[s] / mag;
            // A stamp whose failure is the CALLER's expectation, not an observed one (may_decide): all that is wanted first is whether
            // A + inc I is positive definite after all, and theta1 - |r1| decides that long before theta1 has converged (NOT a rigorous bound:
            // the residual only says that SOME eigenvalue lies within |r1| of theta1; lambda_min can lie below if the block has not captured
            // it.  A stamp decided this way is factored plainly next, and should that fail the iteration runs again: a misjudgement costs
            // time, never a wrong shift -- and only stamps whose failure was EXPECTED, not observed, come here) --
            // lambda_min of a healthy PSF-overlap matrix is rounding noise around zero inside a dense cluster, which this iteration would
            // chase for all its rounds and then hand to the eigensolver.  (From the second Rayleigh-Ritz step on: ten steps bring a
            // lambda_min of the size of -inc out of a random block beyond doubt.)  theta1 is then no eigenvalue: `decided` says so.
            if (may_decide[s] && round >= 1 && inc_failed[s] > 0.0 && (th1 - r1) + inc_failed[s] > 1e-3 * inc_failed[s]) {
                conv[s] = 1; decided[s] = 1; lastrel[s] = rel;
                continue;
            }
            // (the quotient with theta_P is an estimate, not a bound: it ends the iteration only together with the rigorous |r1| <= 1e-6 |theta1|,
            // which keeps the worst case -- theta1 inside a cluster the block has not separated -- at the rounding level of the float32 T)
            if ((bound <= 1e-11 && r1 <= 1e-6 * mag) || (round >= 1 && rel <= 1e-11)) { conv[s] = 1; lastrel[s] = rel; continue; }
            // a shift just above |theta| (theta >= lambda_min: it must exceed |theta| by more than theta's error)
            // a first shift that is already close (a good hint): no second factorisation, the rounds go on where they are; a step multiplies
            // the error by ((lambda_min + sigma) / (|lambda_min| + lambda_min + sigma))^2 (the bulk of the spectrum is |lambda_min| away)
            const double close = theta[s] < 0.0 ? (sigma[s] + theta[s]) / mag : 1e300;
            if (!fine[s] && close > 0.0 && close <= 0.25) {
                fine[s] = 1;
                eta[s] = close;
                const double c = (close / (bulk + close)) * (close / (bulk + close));
                steps_wanted[s] = (int)std::min(6.0, std::max(1.0, ceil(log(std::max(1e-11 / std::max(bound, 1e-300), 1e-300)) / log(c))));
            }
            if (!fine[s] && theta[s] < 0.0 && sigma[s] > 4.0 * (mag + r1) && !(bound <= 0.15)) {
                // a first shift far above what is needed (the x 8 ladder overshot, or a hint from another regime): the block converges by
                // (1 - |lambda_min| / sigma)^2 per step there.  lambda_min >= theta1 - |r1| (rigorous): one factorisation at twice that, still coarse
                eta[s] = 1.0 + 2.0 * r1 / mag;
                refac[s] = 1; any_refac = true;
            } else if (!fine[s]) {
                if (theta[s] < 0.0 && (bound <= 0.15 || (round >= 1 && rel <= 2e-2))) {
                    fine[s] = 1;
                    eta[s] = std::min(std::max(bound <= 0.15 ? 1.5 * bound : 8.0 * rel, 1e-3), 0.25);
                    refac[s] = 1; any_refac = true;
                    // steps of the first fine round: with e = bound / 3 the error of theta1 and the bulk of the spectrum |theta1| away, the shift
                    // leaves lambda_min + sigma' = 3.5 e |theta1| and a step multiplies the error by (3.5 e)^2: e (12 e^2)^j <= 3e-12
                    steps_wanted[s] = (bound <= 1.5e-2 ? 3 : bound <= 4e-2 ? 4 : bound <= 7e-2 ? 5 : 6) + 1;
                }
            } else if (rel > 0.05 * lastrel[s] && 16.0 * rel < 0.25 * eta[s] && theta[s] < 0.0) {
                eta[s] = std::max(16.0 * rel, 1e-9);
                refac[s] = 1; any_refac = true;
            }
            lastrel[s] = rel;
        }
        for (int t = 0; any_refac; t++) {
            std::vector<double> sg = sigma;
            for (int s : idx) if (refac[s]) sg[s] = -theta[s] * (1.0 + eta[s]);
            IMCOM_TRY(factor(sg, refac, fail));
            nfac++;
            any_refac = false;
            for (int s : idx) {
                if (!refac[s]) continue;
                if (fail[s] == 0) { sigma[s] = sg[s]; refac[s] = 0; }
                else if (t >= 10) { refac[s] = 0; act[s] = 0; }
                else { eta[s] *= 8.0; any_refac = true; }
            }
            if (any_refac) nfac_failed++;
        }
        rounds_run = round + 1;
        if (dbg) {
            const int s = idx[0];
            fprintf(stderr, "[lmin] round %d (%d steps): stamp %d theta %.15e (prev %.15e) sigma %.6e eta %.3e fine %d conv %d   |r1| %.3e  bound %.3e (of |theta|)\n", round,
                    iters, s, theta[s], prev[s], sigma[s], eta[s], (int)fine[s], (int)conv[s], est_simple[s], est[s] / std::max(fabs(theta[s]), 1e-300));
            double rmin = 1e300, rmax = 0.0, bmin = 1e300, bmax = 0.0, smin = 1e300, smax_ = 0.0;
            int nfine = 0, nconv = 0, nrun = 0;
            for (int q : idx) {
                if (!run[q]) continue;
                const double mag = std::max(fabs(theta[q]), 1e-300);
                nrun++; nfine += fine[q]; nconv += conv[q];
                rmin = std::min(rmin, lastrel[q]); rmax = std::max(rmax, lastrel[q]);
                bmin = std::min(bmin, est[q] / mag); bmax = std::max(bmax, est[q] / mag);
                smin = std::min(smin, est_simple[q] / mag); smax_ = std::max(smax_, est_simple[q] / mag);
            }
            fprintf(stderr, "[lmin]   %d stamps ran: change of theta %.2e .. %.2e, bound %.2e .. %.2e, |r1| / |theta| %.2e .. %.2e, %d fine, %d converged\n", nrun, rmin, rmax, bmin,
                    bmax, smin, smax_, nfine, nconv);
        }
    }
    if (dbg) for (int s : idx) if (conv[s] && dbg_r1[s] > 0.0) {
        const double d = dbg_th[s] - theta[s];
        fprintf(stderr, "[lmin0] stamp %d theta0 %.9e final %.15e err %.3e r1 %.3e r1^2/err %.3e th2-th1 %.3e thP-th1 %.3e r2 %.3e\n", s, dbg_th[s], theta[s], d / fabs(theta[s]), dbg_r1[s],
                dbg_r1[s] * dbg_r1[s] / std::max(d, 1e-300), dbg_g2[s], dbg_gP[s], dbg_r2[s]);
    }
    for (int s : idx) {
        ok[s] = act[s] && conv[s];
        if (ok[s]) w0[s] = theta[s];
    }
    if (dbg) {
        double tmin = 1e300, tmax = -1e300;
        for (int s : idx) if (ok[s]) { tmin = std::min(tmin, w0[s]); tmax = std::max(tmax, w0[s]); }
        int nok = 0;
        for (int s : idx) nok += ok[s] ? 1 : 0;
        fprintf(stderr, "[lmin] %zu stamps: %d factorisations (%d of them failed for some stamp), %d rounds; lambda_min %.6e .. %.6e; %d without an answer (the eigensolver's)\n", idx.size(), nfac,
                nfac_failed, rounds_run, tmin, tmax, (int)idx.size() - nok);
    }
    ctx->ws_used = mark;
    return IMCOM_OK;
}

// before_solve (optional): called once, after the first factorisation's launches have been queued and before the first launch
// that reads Bt -- the host-buffer entry uploads -B/2 there, behind the factorisation instead of in front of it.
// what the coaddition needs besides T (coadd.py:1294-1363), for the entries that solve and coadd in one call
struct CoaddArgs {
    int n2f, fade, n2, n_inframe, n_expo;
    const float *indata;
    const int *expo;
    float *outimage;
    double *Tsum_stamp, *Tsum_inpix, *Neff;
};

static bool coadd_fusable(int nv, int fade)
{
    return !env_is("IMCOM_SOLVE_UNFUSED") && nv == 1 && fade == 0;  // one kappa node: T is final in the backward launches; no taper to apply to it first
}

static size_t coadd_fuse_bytes(int batch, int Np, int m, int mp, int nv, const CoaddArgs *co)
{
    if (!co) return 0;
    size_t t = (size_t)batch * m * co->n_expo * 8 + 512;  // Tsum_image
    if (coadd_fusable(nv, co->fade)) t += (size_t)batch * 2 * (Np / NB) * (co->n_expo + co->n_inframe) * mp * 8 + 512;
    return t;
}

// redo_host (optional, one kappa node only): per stamp 0 = leave the stamp and its outputs alone, 1 = solve it, 2 = solve it knowing that
// the factorisation of A + kappa I fails (imcom_solve_chol_resident_end OBSERVED it: straight to the repair), 3 = the same as the caller's
// EXPECTATION (the stamps before it failed): straight to the repair, but the smallest-eigenvalue iteration may find that A + kappa I is
// positive definite after all and end early (may_decide), the stamp is then factored plainly.  An observed failure never takes that
// shortcut (the bound it rests on is not rigorous, and for an observed failure it could only cost a second iteration).
// With ONE kappa node an attempt after the first works on the stamps whose factorisation failed and on nothing else: the launches
// see the other stamps with no blocks at all, and their outputs stay what the first attempt wrote (a batch of 256 in which one
// factorisation fails used to be factored and solved three times over).
static int chol_core(imcom_ctx *ctx, int batch, const int *n_host, int Np, int m, int mp, const double *A,
                     const double *Bt, const double *C_host, const double *kappaC_host, int nv, double ucmin,
                     double smax, float *Tt, float *UC, float *Sigma, float *kappa, int *info_host,
                     const std::function<int()> &before_solve = nullptr, const CoaddArgs *co = nullptr, bool defer = false,
                     const int *redo_host = nullptr)
{
    bool bt_ready = !before_solve;
    ctx->last_repair_count = 0;
    const int nbmax_all = Np / NB;
    const int pb = nodes_per_pass(batch, mp, nv), eb = batch * pb;  // nodes per pass, stamps x nodes of a pass
    const bool masked = nv == 1;  // (pb == 1 then)
    IMCOM_REQUIRE(!redo_host || masked, "a redo mask needs a single kappa node");
    double *L = (double *)ws_take(ctx, (size_t)eb * Np * Np * 8);
    double *Dinv = (double *)ws_take(ctx, (size_t)eb * nbmax_all * NB * NB * 8);
    const long node_stride = (long)batch * Np * mp;
    double *Y = (double *)ws_take(ctx, (size_t)nv * node_stride * 8);
    double *dshift = (double *)ws_take(ctx, (size_t)eb * Np * 8);
    int *ints = (int *)ws_take(ctx, (size_t)eb * 4 * 3 + (size_t)batch * 4 * nv);
    int *mints = (int *)ws_take(ctx, (size_t)batch * 4 * 4);
    double *inc = (double *)ws_take(ctx, (size_t)eb * MAX_INC_HOST * 8);
    double *dbl = (double *)ws_take(ctx, (size_t)batch * 8 * 2);
    double *kappaC_dev = (double *)ws_take(ctx, (size_t)nv * 8);
    double *Dp = nullptr, *Npq = nullptr, *W = nullptr;
    if (nv > 1) {
        Dp = (double *)ws_take(ctx, (size_t)batch * m * nv * 8);
        Npq = (double *)ws_take(ctx, (size_t)batch * m * nv * nv * 8);
        W = (double *)ws_take(ctx, (size_t)batch * m * nv * 8);
    }
    const size_t pbytes = splitk_bytes(eb, Np, mp);
    double *partial = pbytes ? (double *)ws_take(ctx, pbytes) : nullptr;
    const int parts_solve = partial ? splitk_parts(eb, mp / NB) : 1;
    // single kappa with the diagonal blocks fused into the solve launches: the launches leave T (float32) and the column sums
    // the maps need behind, and the pass of finalize_single_kernel over X and -B/2 (27 GB per 256 cfg-2 stamps) is not needed
    const bool unfused_solve = env_is("IMCOM_SOLVE_UNFUSED");
    double *colsums = (nv == 1 && !unfused_solve) ? (double *)ws_take(ctx, (size_t)batch * 2 * nbmax_all * mp * 8 * 2) : nullptr;
    double *Dpart = colsums, *Npart = colsums ? colsums + (size_t)batch * 2 * nbmax_all * mp : nullptr;
    // the coaddition of the same call: its sums ride in the backward launches when T is final there (else the stand-alone epilogue)
    CoaddFuse cfuse;
    double *Tsum_image = nullptr;
    if (co) {
        Tsum_image = (double *)ws_take(ctx, (size_t)batch * m * co->n_expo * 8);
        if (colsums && coadd_fusable(nv, co->fade)) {
            cfuse.indata = co->indata; cfuse.expo = co->expo; cfuse.n_inframe = co->n_inframe; cfuse.n_expo = co->n_expo;
            cfuse.Epart = (double *)ws_take(ctx, (size_t)batch * 2 * nbmax_all * (co->n_expo + co->n_inframe) * mp * 8);
        }
        if (!Tsum_image || (colsums && coadd_fusable(nv, co->fade) && !cfuse.Epart)) return ws_short("coaddition");
    }
    if (!L || !Dinv || !Y || !dshift || !ints || !mints || !inc || !dbl || !kappaC_dev || (nv > 1 && (!Dp || !Npq || !W)) || (pbytes && !partial) || (nv == 1 && !unfused_solve && !colsums))
        return ws_short("Cholesky");
    const size_t ws_after_plan = ctx->ws_used;  // (the repair's own scratch is taken from here on and handed back)
    int *n_dev = ints, *nblk_dev = ints + eb, *ninc_dev = ints + 2 * eb, *fail_dev = ints + 3 * eb;  // n, nblk, ninc [eb]; fail[nv][batch]
    int *fac_dev = mints, *nblk_fac = mints + batch, *nblk_sol = mints + 2 * batch, *act_dev = mints + 3 * batch;  // one kappa node: this attempt's stamps
    double *kap_dev = dbl, *C_dev = dbl + batch;

    std::vector<int> nblk(batch), ninc(batch, 0), fail((size_t)nv * batch);
    std::vector<double> inc_h((size_t)batch * MAX_INC_HOST, 0.0), kap_h(batch), rep(batch, 0.0);
    std::vector<char> repaired((size_t)nv * batch, 0), have_w0(batch, 0);
    std::vector<char> active(batch, 1), known(batch, 0), expected(batch, 0);  // the stamps of the coming attempt; stamps whose first factorisation is known
                                                                            // to fail; ... of which by the caller's expectation only (redo code 3)
    std::vector<char> expected_only(batch, 0);            // ... of which the eigenvalue says that they do not fail after all
    int nbmax = 0;
    for (int s = 0; s < batch; s++) {
        IMCOM_REQUIRE(n_host[s] >= 0 && n_host[s] <= Np, "n[%d]=%d outside [0,%d]", s, n_host[s], Np);
        nblk[s] = (n_host[s] + NB - 1) / NB;
        if (nblk[s] > nbmax) nbmax = nblk[s];
        if (redo_host) { active[s] = redo_host[s] != 0; known[s] = redo_host[s] >= 2; expected[s] = redo_host[s] == 3; }
        if (active[s]) info_host[s] = 0;
    }
    for (int q = 0; q < pb; q++) {  // the stamps of a pass: node-major copies
        IMCOM_TRY(upload(ctx, n_dev + q * batch, n_host, batch));
        IMCOM_TRY(upload(ctx, nblk_dev + q * batch, nblk.data(), batch));
    }
    IMCOM_TRY(upload(ctx, C_dev, C_host, batch));
    IMCOM_TRY(upload(ctx, kappaC_dev, kappaC_host, nv));

    // one factorisation over the stamps of `mask` with the diagonal A_ii + shift[s] (the smallest-eigenvalue iteration's trial
    // factorisations: lambda_min_subspace), flags read back
    auto factor_masked = [&](const std::vector<double> &shift, const std::vector<char> &mask, std::vector<int> &fail_h) -> int {
        std::vector<int> nb(batch), one(batch, 1);
        std::vector<double> ih((size_t)batch * MAX_INC_HOST, 0.0);
        int nbm = 0;
        for (int s = 0; s < batch; s++) {
            nb[s] = mask[s] ? nblk[s] : 0;
            nbm = std::max(nbm, nb[s]);
            ih[(size_t)s * MAX_INC_HOST] = shift[s];
        }
        IMCOM_TRY(upload(ctx, nblk_fac, nb.data(), (size_t)batch));
        IMCOM_TRY(upload(ctx, inc, ih.data(), ih.size()));
        IMCOM_TRY(upload(ctx, ninc_dev, one.data(), (size_t)batch));
        IMCOM_TRY(launch_diag_shift(ctx, A, Np, inc, ninc_dev, dshift, batch));
        IMCOM_HIP_CHECK(hipMemsetAsync(fail_dev, 0, (size_t)batch * 4, ctx->stream));
        for (int k = 0; k < nbm; k++) {
            IMCOM_TRY(launch_chol_update(ctx, A, L, Np, k, nbm, batch, batch, nblk_fac, dshift, partial, partial ? splitk_parts(batch, nbm - k) : 1));
            IMCOM_TRY(launch_chol_diag(ctx, L, Dinv, Np, k, batch, nblk_fac, fail_dev));
            IMCOM_TRY(launch_chol_trsm(ctx, L, Dinv, Np, k, nbm, batch, nblk_fac));
        }
        fail_h.assign(batch, 0);
        IMCOM_HIP_CHECK(hipMemcpyAsync(fail_h.data(), fail_dev, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return IMCOM_OK;
    };
    // Yv = (L L^T)^-1 Xv on blocks of 16 vectors (lmin_skinny.hip) for the stamps of `mask`: one workgroup per stamp, both sweeps in one
    // launch -- or, for few stamps, two launches per block row with the sums dealt to many workgroups (part: their scratch).
    // (Per-block-row launches: 1.8 ms of launches per solve + 44 us per production stamp at 7 TB/s; a workgroup per stamp: 12 ms whatever
    // the count -- they meet near 200 stamps, and at 168 the single launch is 2 % ahead on the wall clock.)
    auto solve_block = [&](const std::vector<char> &mask, const double *Xv, double *Yv, double *part) -> int {
        std::vector<int> nb(batch);
        int nbm = 0, cnt = 0;
        for (int s = 0; s < batch; s++) { nb[s] = mask[s] ? nblk[s] : 0; nbm = std::max(nbm, nb[s]); cnt += mask[s] ? 1 : 0; }
        IMCOM_TRY(upload(ctx, nblk_sol, nb.data(), (size_t)batch));
        if (cnt <= env_int("IMCOM_LMIN_FEW_MAX", 128) && part && skinny_few_partial_doubles(batch) <= (size_t)batch * 8 * NB * NB)
            return launch_skinny_solve_few(ctx, L, Dinv, Xv, Yv, Np, nblk_sol, nbm, batch, part);
        return launch_skinny_solve(ctx, L, Dinv, Xv, Yv, Np, nblk_sol, batch);
    };

    for (int attempt = 0;; attempt++) {
        IMCOM_HIP_CHECK(hipMemsetAsync(fail_dev, 0, (size_t)nv * batch * 4, ctx->stream));
        const int *nb_fac = nblk_dev, *nb_sol = nblk_dev, *act_fin = nullptr;
        std::vector<char> fac(batch, 1);  // the stamps this attempt factors
        if (masked) {
            std::vector<int> f_i(batch), nb_i(batch);
            for (int s = 0; s < batch; s++) {
                fac[s] = active[s] && !(attempt == 0 && known[s]);
                f_i[s] = fac[s];
                nb_i[s] = fac[s] ? nblk[s] : 0;
            }
            IMCOM_TRY(upload(ctx, fac_dev, f_i.data(), (size_t)batch));
            IMCOM_TRY(upload(ctx, nblk_fac, nb_i.data(), (size_t)batch));
            nb_fac = nblk_fac; nb_sol = nblk_sol; act_fin = act_dev;
        }
        bool any_fac = false;
        for (int s = 0; s < batch; s++) any_fac |= fac[s] != 0;
        for (int p0 = 0; any_fac && p0 < nv; p0 += pb) {
            for (int q = 0; q < pb; q++) {
                const int p = p0 + q;
                // the diagonal of AA at node p as the reference builds it: a sequence of in-place adds
                // (lakernel.py:298 single kappa; 356 node differences; 268/277 repair add and restore)
                for (int s = 0; s < batch; s++) {
                    double *ih = &inc_h[(size_t)s * MAX_INC_HOST];
                    int c = 0;
                    if (nv == 1) { if (kappaC_host[0] * C_host[s] != 0.0) ih[c++] = kappaC_host[0] * C_host[s]; }
                    else
                        for (int qq = 0; qq <= p; qq++) {
                            ih[c++] = kappaC_host[qq] * C_host[s] - (qq > 0 ? kappaC_host[qq - 1] * C_host[s] : 0.0);
                            if (qq < p && repaired[(size_t)qq * batch + s]) { ih[c++] = rep[s]; ih[c++] = -rep[s]; }
                        }
                    if (repaired[(size_t)p * batch + s]) ih[c++] = rep[s];  // c <= 3 nv <= MAX_INC: nv <= CHOL_MAXNV is checked at entry
                    ninc[s] = c;
                    kap_h[s] = kappaC_host[p] * C_host[s];
                }
                IMCOM_TRY(upload(ctx, inc + (size_t)q * batch * MAX_INC_HOST, inc_h.data(), inc_h.size()));
                IMCOM_TRY(upload(ctx, ninc_dev + q * batch, ninc.data(), batch));
                if (q == 0) IMCOM_TRY(upload(ctx, kap_dev, kap_h.data(), batch));  // used by the single-kappa finalize only
                IMCOM_TRY(launch_diag_shift(ctx, A, Np, inc + (size_t)q * batch * MAX_INC_HOST, ninc_dev + q * batch, dshift + (size_t)q * batch * Np, batch));
            }
            int *failp = fail_dev + (size_t)p0 * batch;
            for (int k = 0; k < nbmax; k++) {
                { ProfScope ps(ctx, "chol_gemm"); IMCOM_TRY(launch_chol_update(ctx, A, L, Np, k, nbmax, eb, batch, nb_fac, dshift, partial, partial ? splitk_parts(eb, nbmax - k) : 1)); }
                { ProfScope ps(ctx, "chol_diag"); IMCOM_TRY(launch_chol_diag(ctx, L, Dinv, Np, k, eb, nb_fac, failp)); }
                { ProfScope ps(ctx, "chol_gemm"); IMCOM_TRY(launch_chol_trsm(ctx, L, Dinv, Np, k, nbmax, eb, nb_fac)); }
            }
            // one kappa node: a stamp whose factorisation has just failed is left out of the solves (its tiles return at once)
            if (masked) IMCOM_TRY(launch_solve_mask(ctx, nblk_dev, fac_dev, failp, nblk_sol, act_dev, batch));
            if (!bt_ready) { IMCOM_TRY(before_solve()); bt_ready = true; }
            double *Yp = Y + p0 * node_stride;
            // the diagonal blocks are applied inside the update launches; IMCOM_SOLVE_UNFUSED keeps them apart (A/B runs)
            const double *Dfused = unfused_solve ? nullptr : Dinv;
            for (int k = 0; k < nbmax; k++) {
                { ProfScope ps(ctx, "solve_gemm"); IMCOM_TRY(launch_solve_fwd(ctx, L, Bt, Yp, Np, mp, k, eb, batch, nb_sol, n_dev, Dfused, partial, parts_solve, Dpart)); }
                if (unfused_solve) { ProfScope ps(ctx, "solve_dinv"); IMCOM_TRY(launch_solve_dinv(ctx, Dinv, Yp, Np, mp, k, eb, nb_sol, false)); }
            }
            for (int k = nbmax - 1; k >= 0; k--) {
                if (k < nbmax - 1 || !unfused_solve) { ProfScope ps(ctx, "solve_gemm"); IMCOM_TRY(launch_solve_bwd(ctx, L, Yp, Np, mp, k, nbmax, eb, nb_sol, n_dev, Dfused, partial, parts_solve, Npart, Tt, cfuse.Epart ? &cfuse : nullptr)); }
                if (unfused_solve) { ProfScope ps(ctx, "solve_dinv"); IMCOM_TRY(launch_solve_dinv(ctx, Dinv, Yp, Np, mp, k, eb, nb_sol, true)); }
            }
        }
        if (any_fac) {
            ProfScope ps(ctx, "finalize");
            if (nv == 1 && colsums)
                IMCOM_TRY(launch_finalize_fused(ctx, Dpart, Npart, Np, mp, m, n_dev, nblk_dev, kap_dev, C_dev, Tt, UC, Sigma, kappa, batch, act_fin));
            else if (nv == 1)
                IMCOM_TRY(launch_finalize_single(ctx, Y, Bt, Np, mp, m, n_dev, kap_dev, C_dev, Tt, UC, Sigma, kappa, batch, act_fin));
            else
                IMCOM_TRY(launch_multi(ctx, Y, node_stride, Bt, Np, mp, m, n_dev, nv, kappaC_dev, C_dev, ucmin, smax, Dp, Npq, W, Tt, UC, Sigma, kappa, batch));
        }
        if (defer) {
            // imcom_solve_chol_resident_begin: everything of the first attempt is queued; the failure flags travel to page-locked memory
            // behind it (in stream order: before whatever the caller queues next may reuse the workspace) and ..._end reads them
            const size_t cnt = (size_t)nv * batch;
            if (ctx->flag_pin_count < cnt) {
                if (ctx->flag_pin) { IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream)); IMCOM_HIP_CHECK(hipHostFree(ctx->flag_pin)); ctx->flag_pin = nullptr; ctx->flag_pin_count = 0; }
                IMCOM_HIP_CHECK(hipHostMalloc((void **)&ctx->flag_pin, std::max<size_t>(cnt, 256) * 4, hipHostMallocDefault));
                ctx->flag_pin_count = std::max<size_t>(cnt, 256);
            }
            IMCOM_HIP_CHECK(hipMemcpyAsync(ctx->flag_pin, fail_dev, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
            IMCOM_TRY(ensure_sync_events(ctx, 3));
            IMCOM_HIP_CHECK(hipEventRecord(ctx->sync_events[2], ctx->stream));
            ctx->deferred_flags = (long)cnt;
            return IMCOM_OK;
        }
        IMCOM_HIP_CHECK(hipMemcpyAsync(fail.data(), fail_dev, fail.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (masked && attempt == 0)
            for (int s = 0; s < batch; s++)
                if (active[s] && known[s]) fail[s] = 1;  // (the caller's knowledge stands for the factorisation that was not repeated)
        bool any = false;
        std::vector<int> need;  // stamps whose smallest eigenvalue is wanted: w, v = eigh(A); shift by |w[0]| + 1e-16
        for (int s = 0; s < batch; s++) {
            bool f = false;
            for (int p = 0; p < nv; p++) {
                if (fail[(size_t)p * batch + s] == 0) continue;
                if (repaired[(size_t)p * batch + s]) {
                    set_error("stamp %d node %d: Cholesky failed again after the lakernel.py:262-279 repair (pivot %d)", s, p,
                              fail[(size_t)p * batch + s]);
                    return IMCOM_ERR_NUMERIC;
                }
                f = true;
            }
            if (f && !have_w0[s]) need.push_back(s);
        }
        if (!need.empty()) {
            ProfScope ps(ctx, "eigen_repair");
            std::vector<double> w0v(batch, 0.0);
            std::vector<char> got(batch, 0);
            std::vector<int> big;
            std::vector<char> may_decide(batch, 0), decided(batch, 0);
            if (lmin_subspace_enabled())
                for (int s : need)
                    if (n_host[s] >= LMIN_MIN_N) big.push_back(s);
            if (!big.empty()) {
                // the largest diagonal increment whose factorisation failed: the first trial shift is four times that
                std::vector<double> incf(batch, 0.0);
                for (int s : big)
                    for (int p = 0; p < nv; p++)
                        if (fail[(size_t)p * batch + s] != 0) incf[s] = std::max(incf[s], kappaC_host[p] * C_host[s]);
                ctx->ws_used = ws_after_plan;
                for (int s : big) may_decide[s] = masked && attempt == 0 && expected[s];
                IMCOM_TRY(lambda_min_subspace(ctx, batch, n_host, n_dev, Np, A, big, incf, ctx->repair_hint, may_decide, decided, factor_masked, solve_block, w0v, got));
                ctx->ws_used = ws_after_plan;
            }
            std::vector<int> rest;
            for (int s : need)
                if (!got[s]) rest.push_back(s);
            for (size_t g0 = 0; g0 < rest.size(); g0 += REPAIR_GROUP) {
                const int cnt = (int)std::min<size_t>(REPAIR_GROUP, rest.size() - g0);
                std::vector<double> w0(cnt, 0.0);
                IMCOM_TRY(lambda_min_group(ctx, A, n_host, Np, rest.data() + g0, cnt, w0.data()));
                for (int q = 0; q < cnt; q++) { w0v[rest[g0 + q]] = w0[q]; got[rest[g0 + q]] = 1; }
            }
            for (int s : need) {
                rep[s] = fabs(w0v[s]) + 1e-16;
                have_w0[s] = decided[s] ? 0 : 1;  // (decided: w0v is a lower bound's witness, not the eigenvalue -- should the plain factorisation fail after all, the iteration runs again)
                if (!decided[s]) {
                    ctx->last_w0_min = ctx->last_repair_count ? std::min(ctx->last_w0_min, w0v[s]) : w0v[s];
                    ctx->last_w0_max = ctx->last_repair_count ? std::max(ctx->last_w0_max, w0v[s]) : w0v[s];
                    ctx->last_repair_count++;
                }
                // A stamp whose failure was the CALLER's expectation (redo = 2 without a factorisation having failed here): the smallest
                // eigenvalue says whether A + kappa I is positive definite after all.  If it clearly is (w0 + kappa above 1e-6 kappa: the
                // eigenvalue is good to 1e-11) the reference's cholesky() succeeds and nothing is repaired: the stamp is factored plainly in
                // the next attempt -- and repaired then, should that factorisation fail in spite of the eigenvalue.
                const double kap_s = kappaC_host[0] * C_host[s];
                if (masked && attempt == 0 && expected[s] && w0v[s] + kap_s > 1e-6 * fabs(kap_s)) expected_only[s] = 1;
            }
        }
        std::vector<char> next(batch, 0);
        for (int p = 0; p < nv; p++)
            for (int s = 0; s < batch; s++) {
                if (fail[(size_t)p * batch + s] == 0) continue;
                next[s] = 1;
                any = true;
                if (masked && attempt == 0 && expected_only[s]) continue;  // (solved in the next attempt, without the repair)
                repaired[(size_t)p * batch + s] = 1;
                if (info_host[s] == 0) info_host[s] = p + 1;
            }
        if (!any) break;
        if (masked) active = next;  // the next attempt: the stamps that failed, nothing else
        IMCOM_REQUIRE(attempt <= nv + 1, "repair loop did not terminate");
    }
    if (co) {
        ProfScope ps(ctx, "epilogue");
        if (cfuse.Epart)
            IMCOM_TRY(launch_coadd_from_partials(ctx, batch, n_dev, nblk_dev, Np, m, mp, co->n2, cfuse, co->outimage, Tsum_image, co->Tsum_stamp, co->Tsum_inpix,
                                                 co->Neff));
        else
            IMCOM_TRY(launch_epilogue(ctx, batch, n_dev, Np, m, mp, co->n2f, co->fade, co->n2, Tt, co->indata, co->n_inframe, co->expo, co->n_expo, co->outimage,
                                      Tsum_image, co->Tsum_stamp, co->Tsum_inpix, co->Neff));
    }
    return IMCOM_OK;
}

// The argument rules of the four resident Cholesky entries.  `more`: the entry's own pointers are there (info, redo); `redo`: one
// kappa node only (imcom_solve_chol_resident_redo); `co`: the coaddition's rules too (imcom_solve_chol_resident_coadd).
static int resident_args(int batch, const int *n_host, int ldn, int m, int ldm, const double *A, const double *Bt, const double *C_host,
                         const double *kappaC_host, int nv, const float *Tt, const float *UC, const float *Sigma, const float *kappa, bool more,
                         bool redo, const CoaddArgs *co)
{
    IMCOM_REQUIRE(batch >= 1 && n_host && A && Bt && C_host && kappaC_host && Tt && UC && Sigma && kappa && more, "null pointer");
    if (co)
        IMCOM_REQUIRE(co->indata && co->expo && co->outimage && co->Tsum_stamp && co->Tsum_inpix && co->Neff, "null pointer (coaddition)");
    IMCOM_REQUIRE(ldn >= NB && ldn % NB == 0 && ldm % NB == 0 && m >= 1 && m <= ldm && (redo || nv >= 1), "ldn=%d / ldm=%d must be multiples of %d", ldn, ldm, NB);
    if (redo) IMCOM_REQUIRE(nv == 1, "imcom_solve_chol_resident_redo: one kappa node (nv=%d: call imcom_solve_chol_resident)", nv);
    else IMCOM_REQUIRE(nv <= CHOL_MAXNV, "nv=%d kappa nodes: at most %d", nv, CHOL_MAXNV);
    if (co) {
        IMCOM_REQUIRE(m == co->n2f * co->n2f && co->n_inframe >= 1 && co->n_expo >= 1 && co->fade >= 0 && co->n2 >= 1, "bad sizes (coaddition)");
        IMCOM_REQUIRE(co->fade == 0, "imcom_solve_chol_resident_coadd: fade = %d -- the map tapers of coadd.py:1118-1122 come between the solve and the coaddition: "
                                     "call imcom_solve_chol_resident, imcom_trapezoid_f32, imcom_coadd_epilogue", co->fade);
    }
    return IMCOM_OK;
}

// A begin whose end never came (the caller failed in between): its work is waited for and forgotten.
static int drain_begin(imcom_ctx *ctx)
{
    if (ctx->deferred_flags != 0) {
        IMCOM_HIP_CHECK(hipEventSynchronize(ctx->sync_events[2]));
        ctx->deferred_flags = 0;
    }
    return IMCOM_OK;
}

// The host Cholesky entries upload -B/2 on the context's second queue while the factorisation runs.  The copy lands in workspace that
// kernels of an EARLIER, un-synchronised device-mode call on this context may still be using: it waits for the point the main stream had
// reached when the entry began (mark_entry: sync_events[1]) -- not for the entry's own factorisation, behind which it is meant to hide --
// and the main stream waits for the copy (sync_events[0]) before it packs.
static int mark_entry(imcom_ctx *ctx)
{
    IMCOM_TRY(ensure_sync_events(ctx, 2));
    IMCOM_HIP_CHECK(hipEventRecord(ctx->sync_events[1], ctx->stream));  // everything earlier calls left on the main stream
    return IMCOM_OK;
}

static int upload_behind_entry(imcom_ctx *ctx, const std::function<int(hipStream_t)> &copies)
{
    IMCOM_TRY(ensure_aux(ctx));
    IMCOM_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->sync_events[1], 0));
    IMCOM_TRY(copies(ctx->aux_stream));
    IMCOM_HIP_CHECK(hipEventRecord(ctx->sync_events[0], ctx->aux_stream));
    IMCOM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->sync_events[0], 0));
    return IMCOM_OK;
}

}  // namespace imcom

using namespace imcom;

extern "C" {

// Bytes of workspace imcom_solve_chol_resident (and _begin / _redo) takes: pure arithmetic, for a planner
int imcom_solve_chol_workspace(int batch, int ldn, int m, int ldm, int nv, size_t *bytes)
{
    IMCOM_REQUIRE(batch >= 1 && ldn >= NB && ldn % NB == 0 && ldm >= NB && ldm % NB == 0 && m >= 1 && m <= ldm && nv >= 1 && nv <= CHOL_MAXNV && bytes,
                  "bad sizes (ldn, ldm multiples of 128)");
    *bytes = chol_core_bytes(batch, ldn, m, ldm, nv);
    return IMCOM_OK;
}

int imcom_solve_chol(imcom_ctx *ctx, int batch, const int *n, int ldn, int m, const double *A, const double *mBhalf,
                     const double *C, const double *kappaC, int nv, double ucmin, double smax, float *T, float *UC,
                     float *Sigma, float *kappa, int *info, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && n && C && kappaC && UC && Sigma && kappa && info, "null pointer / empty batch");
    IMCOM_REQUIRE(m >= 1 && nv >= 1 && ldn >= 0, "bad sizes");
    IMCOM_REQUIRE(nv <= CHOL_MAXNV, "nv=%d kappa nodes: at most %d", nv, CHOL_MAXNV);
    int nmax;
    IMCOM_TRY(batch_sizes(n, batch, ldn, &nmax));
    IMCOM_REQUIRE(nmax == 0 || (A && mBhalf && T), "null matrix pointer");
    Stage st(ctx, memspace, __func__);
    const int Np = (int)align_up((size_t)(nmax > 0 ? nmax : 1), NB), mp = (int)align_up((size_t)m, NB);
    const size_t szA = (size_t)batch * ldn * ldn, szB = (size_t)batch * m * ldn, szM = (size_t)batch * m;
    WsPlan plan;
    st.plan(plan, {szA * 8, szB * 8, szB * 4, szM * 4, szM * 4, szM * 4});
    plan.add((size_t)batch * Np * Np * 8);  // Ap
    plan.add((size_t)batch * Np * mp * 8);  // Bt
    plan.add((size_t)batch * Np * mp * 4);  // Tt
    plan.add((size_t)batch * 4);            // n
    IMCOM_TRY(ws_reserve(ctx, plan.total + chol_core_bytes(batch, Np, m, mp, nv) + 8192));
    const double *A_d;
    double *B_d;
    float *T_d, *UC_d, *Sig_d, *kap_d;
    IMCOM_TRY(st.in(A, szA, &A_d));
    // -B/2 is not needed before the triangular solves: from host memory it is uploaded on the context's second queue while the
    // factorisation runs (a third of a stamp's 100 MB over PCIe moves behind 3 ms of Cholesky)
    IMCOM_TRY(st.out((double *)mBhalf, szB, &B_d));
    IMCOM_TRY(st.out(T, szB, &T_d));
    IMCOM_TRY(st.out(UC, szM, &UC_d));
    IMCOM_TRY(st.out(Sigma, szM, &Sig_d));
    IMCOM_TRY(st.out(kappa, szM, &kap_d));
    double *Ap = (double *)ws_take(ctx, (size_t)batch * Np * Np * 8);
    double *Bt = (double *)ws_take(ctx, (size_t)batch * Np * mp * 8);
    float *Tt = (float *)ws_take(ctx, (size_t)batch * Np * mp * 4);
    int *n_dev = (int *)ws_take(ctx, (size_t)batch * 4);
    if (!Ap || !Bt || !Tt || !n_dev) return ws_short(__func__);
    IMCOM_TRY(upload(ctx, n_dev, n, batch));
    {
        ProfScope ps(ctx, "pack");
        IMCOM_TRY(launch_pack_A(ctx, A_d, ldn, n_dev, Ap, Np, batch));
    }
    const bool aux_B = st.host && szB > 0;
    if (aux_B) IMCOM_TRY(mark_entry(ctx));
    auto stage_B = [&]() -> int {
        if (aux_B) IMCOM_TRY(upload_behind_entry(ctx, [&](hipStream_t aux) -> int {
            IMCOM_HIP_CHECK(hipMemcpyAsync(B_d, mBhalf, szB * 8, hipMemcpyHostToDevice, aux));
            return IMCOM_OK;
        }));
        ProfScope ps(ctx, "pack");
        return launch_pack_Bt(ctx, B_d, ldn, m, n_dev, Bt, Np, mp, batch);
    };
    // imcom_ctx_set_repair_expect: the caller has seen the factorisation of A + kappa I fail on the stamps before these (the reference's
    // production shape: every stamp) -- straight to _cholesky_wrapper's repair, as the resident path's redo code 2
    const std::vector<int> expect_all(batch, 3);
    const int rc_core = chol_core(ctx, batch, n, Np, m, mp, Ap, Bt, C, kappaC, nv, ucmin, smax, Tt, UC_d, Sig_d, kap_d, info, stage_B, nullptr, false,
                                  (ctx->repair_expect && nv == 1) ? expect_all.data() : nullptr);
    if (rc_core != IMCOM_OK) {
        if (st.host && ctx->aux_stream) hipStreamSynchronize(ctx->aux_stream);  // nothing of this call may still be copying into the workspace
        return rc_core;
    }
    if (ldn > 0) { ProfScope ps(ctx, "pack"); IMCOM_TRY(launch_unpack_T(ctx, Tt, Np, mp, n_dev, m, T_d, ldn, batch)); }
    IMCOM_TRY(st.back(T, T_d, szB));
    IMCOM_TRY(st.back(UC, UC_d, szM));
    IMCOM_TRY(st.back(Sigma, Sig_d, szM));
    IMCOM_TRY(st.back(kappa, kap_d, szM));
    return st.done();
}

// The same kernel for SEVERAL OutStamps per call, each with its own host arrays (the four OutStamps of a 2 x 2 group, say): one
// batched factorisation / solve for all of them, -B/2 uploaded behind the factorisation.  See imcom_hip.h.
int imcom_solve_chol_stamps(imcom_ctx *ctx, int nst, const int *n, int m, const double *const *A, const double *const *mBhalf,
                            const double *C, const double *kappaC, int nv, double ucmin, double smax, float *const *T,
                            float *const *UC, float *const *Sigma, float *const *kappa, int *info)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(nst >= 1 && n && A && mBhalf && C && kappaC && T && UC && Sigma && kappa && info, "null pointer / no stamps");
    IMCOM_REQUIRE(m >= 1 && nv >= 1, "bad sizes");
    IMCOM_REQUIRE(nv <= CHOL_MAXNV, "nv=%d kappa nodes: at most %d", nv, CHOL_MAXNV);
    int nmax = 0;
    size_t totA = 0, totB = 0;
    for (int s = 0; s < nst; s++) {
        IMCOM_REQUIRE(n[s] >= 0, "n[%d]=%d", s, n[s]);
        IMCOM_REQUIRE(UC[s] && Sigma[s] && kappa[s] && (n[s] == 0 || (A[s] && mBhalf[s] && T[s])), "null pointer for stamp %d", s);
        nmax = std::max(nmax, n[s]);
        totA += align_up((size_t)n[s] * n[s], 32);
        totB += align_up((size_t)m * n[s], 32);
    }
    const int Np = (int)align_up((size_t)(nmax > 0 ? nmax : 1), NB), mp = (int)align_up((size_t)m, NB);
    const size_t szM = (size_t)nst * m;
    WsPlan plan;
    plan.add(totA * 8); plan.add(totB * 8); plan.add(totB * 4); plan.add(szM * 4 * 3);
    plan.add((size_t)nst * Np * Np * 8);  // Ap
    plan.add((size_t)nst * Np * mp * 8);  // Bt
    plan.add((size_t)nst * Np * mp * 4);  // Tt
    plan.add((size_t)nst * 4);            // n
    IMCOM_TRY(ws_reserve(ctx, plan.total + chol_core_bytes(nst, Np, m, mp, nv) + 8192));
    double *rawA = (double *)ws_take(ctx, totA * 8), *rawB = (double *)ws_take(ctx, totB * 8);
    float *rawT = (float *)ws_take(ctx, totB * 4), *maps = (float *)ws_take(ctx, szM * 4 * 3);
    double *Ap = (double *)ws_take(ctx, (size_t)nst * Np * Np * 8), *Bt = (double *)ws_take(ctx, (size_t)nst * Np * mp * 8);
    float *Tt = (float *)ws_take(ctx, (size_t)nst * Np * mp * 4);
    int *n_dev = (int *)ws_take(ctx, (size_t)nst * 4);
    if (!rawA || !rawB || !rawT || !maps || !Ap || !Bt || !Tt || !n_dev) return ws_short(__func__);
    float *UC_d = maps, *Sig_d = maps + szM, *kap_d = maps + 2 * szM;
    IMCOM_TRY(upload(ctx, n_dev, n, nst));
    std::vector<size_t> offA(nst), offB(nst);
    {
        size_t a = 0, b = 0;
        for (int s = 0; s < nst; s++) { offA[s] = a; offB[s] = b; a += align_up((size_t)n[s] * n[s], 32); b += align_up((size_t)m * n[s], 32); }
    }
    const bool timing = env_is("IMCOM_SEAM_TIMING");  // host-side timeline of the call on stderr (adds a synchronisation)
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    double tA = 0, tB0 = 0, tB1 = 0, tcore = 0, tsync = 0;
    // the system matrices one after the other on the main stream, each packed as soon as it is there
    for (int s = 0; s < nst; s++) {
        if (n[s] == 0) continue;
        IMCOM_HIP_CHECK(hipMemcpyAsync(rawA + offA[s], A[s], (size_t)n[s] * n[s] * 8, hipMemcpyHostToDevice, ctx->stream));
        ProfScope ps(ctx, "pack");
        IMCOM_TRY(launch_pack_A(ctx, rawA + offA[s], n[s], n_dev + s, Ap + (size_t)s * Np * Np, Np, 1));
    }
    IMCOM_TRY(mark_entry(ctx));
    tA = now();
    // -B/2 is called for when the factorisation's launches are queued: its upload (host-blocking from pageable memory) runs on the
    // second queue while the GPU factors
    auto stage_B = [&]() -> int {
        tB0 = now();
        IMCOM_TRY(upload_behind_entry(ctx, [&](hipStream_t aux) -> int {
            for (int s = 0; s < nst; s++)
                if (n[s] > 0) IMCOM_HIP_CHECK(hipMemcpyAsync(rawB + offB[s], mBhalf[s], (size_t)m * n[s] * 8, hipMemcpyHostToDevice, aux));
            return IMCOM_OK;
        }));
        tB1 = now();
        ProfScope ps(ctx, "pack");
        for (int s = 0; s < nst; s++)
            IMCOM_TRY(launch_pack_Bt(ctx, rawB + offB[s], n[s], m, n_dev + s, Bt + (size_t)s * Np * mp, Np, mp, 1));
        return IMCOM_OK;
    };
    const std::vector<int> expect_all(nst, 3);  // (imcom_ctx_set_repair_expect: see imcom_solve_chol)
    const int rc_core = chol_core(ctx, nst, n, Np, m, mp, Ap, Bt, C, kappaC, nv, ucmin, smax, Tt, UC_d, Sig_d, kap_d, info, stage_B, nullptr, false,
                                  (ctx->repair_expect && nv == 1) ? expect_all.data() : nullptr);
    tcore = now();
    if (timing) { hipStreamSynchronize(ctx->stream); tsync = now(); }
    if (rc_core != IMCOM_OK) {
        if (ctx->aux_stream) hipStreamSynchronize(ctx->aux_stream);  // nothing of this call may still be copying into the workspace
        return rc_core;
    }
    for (int s = 0; s < nst; s++) {
        if (n[s] > 0) {
            { ProfScope ps(ctx, "pack"); IMCOM_TRY(launch_unpack_T(ctx, Tt + (size_t)s * Np * mp, Np, mp, n_dev + s, m, rawT + offB[s], n[s], 1)); }
            IMCOM_HIP_CHECK(hipMemcpyAsync(T[s], rawT + offB[s], (size_t)m * n[s] * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        IMCOM_HIP_CHECK(hipMemcpyAsync(UC[s], UC_d + (size_t)s * m, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipMemcpyAsync(Sigma[s], Sig_d + (size_t)s * m, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipMemcpyAsync(kappa[s], kap_d + (size_t)s * m, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (timing)
        fprintf(stderr, "[imcom] solve_chol_stamps nst=%d: A up + pack queued %.2f ms, B copies start %.2f end %.2f, core queued %.2f, compute done %.2f, T down %.2f\n",
                nst, tA - t0, tB0 - t0, tB1 - t0, tcore - t0, tsync - t0, now() - t0);
    return IMCOM_OK;
}

int imcom_solve_chol_resident(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, const double *A,
                              const double *Bt, const double *C_host, const double *kappaC_host, int nv, double ucmin,
                              double smax, float *Tt, float *UC, float *Sigma, float *kappa, int *info_host)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(resident_args(batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, Tt, UC, Sigma, kappa, info_host != nullptr, false, nullptr));
    IMCOM_TRY(ws_reserve(ctx, chol_core_bytes(batch, ldn, m, ldm, nv)));
    return chol_core(ctx, batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, ucmin, smax, Tt, UC, Sigma, kappa, info_host);
}

// The same solve in two halves, for a caller that has host work to do while the device factors and solves (blockrun.coadd_block
// prepares the next pass in between): _begin queues everything of the FIRST attempt and returns; _end waits for it and reads the
// factorisations' failure flags.  All positive definite (the normal case): info = 0, IMCOM_OK, the outputs are final.  Otherwise _end
// returns 1 and has written nothing: the caller runs imcom_solve_chol_resident on the same arguments, which repairs as the reference does
// (lakernel.py:262-279).  Between the two calls the caller may queue other work on the context (it runs behind the solve and may reuse
// the workspace), but no other solve.
int imcom_solve_chol_resident_begin(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, const double *A, const double *Bt,
                                    const double *C_host, const double *kappaC_host, int nv, double ucmin, double smax, float *Tt, float *UC,
                                    float *Sigma, float *kappa)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(resident_args(batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, Tt, UC, Sigma, kappa, true, false, nullptr));
    IMCOM_TRY(drain_begin(ctx));
    IMCOM_TRY(ws_reserve(ctx, chol_core_bytes(batch, ldn, m, ldm, nv)));
    std::vector<int> info(batch, 0);
    return chol_core(ctx, batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, ucmin, smax, Tt, UC, Sigma, kappa, info.data(), nullptr, nullptr, true);
}

int imcom_solve_chol_resident_end(imcom_ctx *ctx, int batch, int *info_host)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(info_host && batch >= 1, "null pointer");
    IMCOM_REQUIRE(ctx->deferred_flags > 0 && ctx->deferred_flags % batch == 0, "imcom_solve_chol_resident_end without a matching begin");
    const long cnt = ctx->deferred_flags;
    ctx->deferred_flags = 0;
    IMCOM_HIP_CHECK(hipEventSynchronize(ctx->sync_events[2]));
    // a factorisation failed: info says whose (info[s] = 1 + the first kappa node that failed), and imcom_solve_chol_resident_redo (one kappa
    // node) or imcom_solve_chol_resident (all stamps again) repairs as the reference does
    bool any = false;
    for (int s = 0; s < batch; s++) info_host[s] = 0;
    for (long q = 0; q < cnt; q++)
        if (ctx->flag_pin[q] != 0) {
            any = true;
            const int s = (int)(q % batch), p = (int)(q / batch);
            if (info_host[s] == 0) info_host[s] = p + 1;
        }
    return any ? 1 : IMCOM_OK;
}

// The solve for SOME stamps of a resident batch (one kappa node): redo_host[s] = 0 leaves stamp s and all its outputs alone, 1 solves
// it, 2 solves it knowing that the plain factorisation fails -- what imcom_solve_chol_resident_end has just reported -- so that the repair
// of lakernel.py:262-279 starts at once.  A batch in which a few factorisations fail costs those stamps again, not the batch.
int imcom_solve_chol_resident_redo(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, const double *A, const double *Bt,
                                   const double *C_host, const double *kappaC_host, int nv, double ucmin, double smax, float *Tt, float *UC,
                                   float *Sigma, float *kappa, const int *redo_host, int *info_host)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(resident_args(batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, Tt, UC, Sigma, kappa, redo_host && info_host, true, nullptr));
    IMCOM_TRY(drain_begin(ctx));
    IMCOM_TRY(ws_reserve(ctx, chol_core_bytes(batch, ldn, m, ldm, nv)));
    return chol_core(ctx, batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, ucmin, smax, Tt, UC, Sigma, kappa, info_host, nullptr, nullptr, false, redo_host);
}

// CholKernel on the device layouts followed by the coaddition of the same stamps, in one call: with one kappa node and fade 0
// the coaddition's sums are taken from the tiles of T while the backward launches still hold them (no pass over T afterwards);
// otherwise the call is imcom_solve_chol_resident + the map tapers' caller + imcom_coadd_epilogue back to back.
int imcom_solve_chol_resident_coadd(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, const double *A, const double *Bt,
                                    const double *C_host, const double *kappaC_host, int nv, double ucmin, double smax, float *Tt, float *UC,
                                    float *Sigma, float *kappa, int *info_host, int n2f, int fade, int n2, const float *indata, int n_inframe,
                                    const int *expo, int n_expo, float *outimage, double *Tsum_stamp, double *Tsum_inpix, double *Neff)
{
    IMCOM_TRY(enter(ctx));
    const CoaddArgs co{n2f, fade, n2, n_inframe, n_expo, indata, expo, outimage, Tsum_stamp, Tsum_inpix, Neff};
    IMCOM_TRY(resident_args(batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, Tt, UC, Sigma, kappa, info_host != nullptr, false, &co));
    IMCOM_TRY(ws_reserve(ctx, chol_core_bytes(batch, ldn, m, ldm, nv) + coadd_fuse_bytes(batch, ldn, m, ldm, nv, &co)));
    return chol_core(ctx, batch, n_host, ldn, m, ldm, A, Bt, C_host, kappaC_host, nv, ucmin, smax, Tt, UC, Sigma, kappa, info_host, nullptr, &co);
}

}  // extern "C"
