// api.hip -- extern "C" entry points of libimcom_hip.so (see include/imcom_hip.h) and the host-side
// orchestration of the batched blocked Cholesky solve.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <functional>

#include "common.h"
#include "launchers.h"
#include "i24_core.h"
#include "quantiles_core.h"
#include "ziggurat_core.h"

namespace imcom {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ws_reserve(imcom_ctx *ctx, size_t bytes)
{
    ctx->ws_used = 0;
    ctx->ws_limit = 0;
    ctx->ws_need = bytes;
    if (bytes <= ctx->ws_bytes) return IMCOM_OK;
    if (ctx->ws_external) {  // the caller owns device memory: say what is needed (imcom_ctx_workspace_needed) and let it decide
        set_error("caller-provided workspace of %zu bytes: this call needs %zu (imcom_ctx_set_workspace)", ctx->ws_bytes, bytes);
        return IMCOM_ERR_NOMEM;
    }
    if (ctx->ws) {
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        IMCOM_HIP_CHECK(hipFree(ctx->ws));
        ctx->ws = nullptr;
        ctx->ws_bytes = 0;
    }
    const size_t want = align_up(bytes + (bytes >> 3), (size_t)1 << 21);
    hipError_t e = hipMalloc((void **)&ctx->ws, want);
    if (e != hipSuccess) {
        set_error("device workspace of %zu bytes: %s", want, hipGetErrorString(e));
        return IMCOM_ERR_NOMEM;
    }
    ctx->ws_bytes = want;
    return IMCOM_OK;
}

void *ws_take(imcom_ctx *ctx, size_t bytes)
{
    const size_t off = align_up(ctx->ws_used, 256);
    const size_t end = ctx->ws_limit ? std::min(ctx->ws_limit, ctx->ws_bytes) : ctx->ws_bytes;
    if (off + bytes > end) return nullptr;  // callers reserve the exact total first
    ctx->ws_used = off + bytes;
    return ctx->ws + off;
}

int ws_short(const char *who)
{
    set_error("internal: workspace plan too small (%s)", who);
    return IMCOM_ERR_NOMEM;
}

int enter(imcom_ctx *ctx)
{
    if (!ctx) { set_error("null context"); return IMCOM_ERR_ARG; }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { set_error("hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e)); return IMCOM_ERR_HIP; }
    return IMCOM_OK;
}

int ensure_sync_events(imcom_ctx *ctx, size_t k)
{
    while (ctx->sync_events.size() < k) {
        hipEvent_t e;
        IMCOM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->sync_events.push_back(e);
    }
    return IMCOM_OK;
}

int batch_sizes(const int *n, int batch, int ldn, int *nmax)
{
    *nmax = 0;
    for (int s = 0; s < batch; s++) {
        IMCOM_REQUIRE(n[s] >= 0 && n[s] <= ldn, "n[%d]=%d exceeds ldn=%d", s, n[s], ldn);
        *nmax = std::max(*nmax, n[s]);
    }
    return IMCOM_OK;
}

ProfScope::ProfScope(imcom_ctx *c, const char *fam, long n, bool fine) : ctx(c), family(fam), launches(n)
{
    if (!ctx->profile || (fine && !ctx->profile_fine)) return;
    auto get = [&]() {
        hipEvent_t e;
        if (!ctx->event_pool.empty()) { e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else hipEventCreate(&e);
        return e;
    };
    start = get();
    stop = get();
    hipEventRecord(start, ctx->stream);
}

ProfScope::~ProfScope()
{
    if (!ctx->profile || !start) return;
    hipEventRecord(stop, ctx->stream);
    ctx->pending.push_back({family, start, stop, launches});
}

int profile_collect(imcom_ctx *ctx)
{
    if (ctx->pending.empty()) return IMCOM_OK;
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (auto &p : ctx->pending) {
        float ms = 0.f;
        IMCOM_HIP_CHECK(hipEventElapsedTime(&ms, p.start, p.stop));
        auto &slot = ctx->prof[p.family];
        slot.ms += ms;
        slot.launches += p.launches;
        ctx->event_pool.push_back(p.start);
        ctx->event_pool.push_back(p.stop);
    }
    ctx->pending.clear();
    return IMCOM_OK;
}

int pin_reserve(imcom_ctx *ctx, size_t bytes)
{
    if (ctx->pin && bytes <= ctx->pin_bytes) return IMCOM_OK;
    if (ctx->pin) { IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream)); IMCOM_HIP_CHECK(hipHostFree(ctx->pin)); ctx->pin = nullptr; }
    IMCOM_HIP_CHECK(hipHostMalloc((void **)&ctx->pin, bytes, hipHostMallocDefault));
    ctx->pin_bytes = bytes;
    ctx->pin_used = 0;
    return IMCOM_OK;
}

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

// The context's second queue, created when a call first needs one (most never do: a stream that exists takes a share of the HIP
// runtime's hardware queues whether or not it carries work).  It carries work that FILLS gaps of the main stream (copies, the Eigen
// path's reflector products): lowest priority, so that a short kernel of the main stream's dependent chain does not queue behind its
// long tiles.
int ensure_aux(imcom_ctx *ctx)
{
    if (ctx->aux_stream) return IMCOM_OK;
    int least = 0, greatest = 0;
    IMCOM_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    // IMCOM_AUX_CUS = k: the second queue confined to k of the CUs (bit i of the mask = CU i / 8 of XCD i % 8), so that the
    // main stream's one-workgroup-per-stamp kernels always find CUs without a product tile on them (A/B runs)
    const int k = env_int("IMCOM_AUX_CUS", 0);
    if (k > 0 && k < ctx->cu_count) {
        std::vector<uint32_t> mask((ctx->cu_count + 31) / 32, 0u);
        for (int i = 0; i < k; i++) mask[i / 32] |= 1u << (i % 32);
        IMCOM_HIP_CHECK(hipExtStreamCreateWithCUMask(&ctx->aux_stream, (uint32_t)mask.size(), mask.data()));
    } else
        IMCOM_HIP_CHECK(hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, least));
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

int imcom_version(void) { return IMCOM_HIP_VERSION; }

const char *imcom_last_error(void) { return g_err; }

int imcom_device_count(int *count)
{
    IMCOM_REQUIRE(count, "null count");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return IMCOM_ERR_HIP; }
    *count = c;
    return IMCOM_OK;
}

int imcom_ctx_create(int device, imcom_ctx **out)
{
    IMCOM_REQUIRE(out, "null ctx pointer");
    *out = nullptr;
    int c = 0;
    IMCOM_HIP_CHECK(hipGetDeviceCount(&c));
    IMCOM_REQUIRE(device >= 0 && device < c, "device %d out of range (have %d)", device, c);
    IMCOM_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    IMCOM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libimcom_hip is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return IMCOM_ERR_UNSUPPORTED;
    }
    imcom_ctx *ctx = new imcom_ctx();
    ctx->device = device;
    ctx->cu_count = prop.multiProcessorCount;
    IMCOM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return IMCOM_OK;
}

int imcom_ctx_destroy(imcom_ctx *ctx)
{
    if (!ctx) return IMCOM_OK;
    (void)enter(ctx);  // (the tear-down goes on whatever the device says)
    hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->pending) { hipEventDestroy(p.start); hipEventDestroy(p.stop); }
    for (auto e : ctx->event_pool) hipEventDestroy(e);
    if (ctx->ws && !ctx->ws_external) hipFree(ctx->ws);
    if (ctx->pin) hipHostFree(ctx->pin);
    for (auto e : ctx->sync_events) hipEventDestroy(e);
    if (ctx->stream_event) hipEventDestroy(ctx->stream_event);
    if (ctx->aux_stream) hipStreamDestroy(ctx->aux_stream);
    for (auto s_ : ctx->sub_streams) hipStreamDestroy(s_);
    for (auto s_ : ctx->part_streams) hipStreamDestroy(s_);
    if (ctx->flag_pin) hipHostFree(ctx->flag_pin);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return IMCOM_OK;
}

int imcom_ctx_set_stream(imcom_ctx *ctx, void *hip_stream)
{
    IMCOM_TRY(enter(ctx));
    hipStream_t next = (hipStream_t)hip_stream;  // NULL = the legacy default stream, which is what torch's default is
    if (next != ctx->stream) {
        // work queued on the old stream may still be using the context's bump workspace, which the next call on the new
        // stream hands out again from offset 0: order the new stream behind it
        if (!ctx->stream_event) IMCOM_HIP_CHECK(hipEventCreateWithFlags(&ctx->stream_event, hipEventDisableTiming));
        IMCOM_HIP_CHECK(hipEventRecord(ctx->stream_event, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamWaitEvent(next, ctx->stream_event, 0));
        ctx->stream = next;
    }
    return IMCOM_OK;
}

int imcom_ctx_sync(imcom_ctx *ctx)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return IMCOM_OK;
}

int imcom_ctx_workspace_bytes(imcom_ctx *ctx, size_t *bytes)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(bytes, "null bytes");
    *bytes = ctx->ws_bytes;
    return IMCOM_OK;
}

int imcom_ctx_workspace_release(imcom_ctx *ctx)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->aux_stream));
    if (ctx->ws && !ctx->ws_external) IMCOM_HIP_CHECK(hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = ctx->ws_used = 0;
    return IMCOM_OK;
}

// One owner for device memory: from this call on the context works in the caller's buffer and never allocates device memory itself
// (a call that needs more returns IMCOM_ERR_NOMEM, imcom_ctx_workspace_needed says how much).  The analogue in the reference is its
// TEMPFILE "virtual memory" knob (psfutil.py:2056-2085): the user decides where the sub-blocks live, not luck.
int imcom_ctx_set_workspace(imcom_ctx *ctx, void *ptr, size_t bytes)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE((ptr != nullptr) == (bytes > 0), "workspace pointer and size must come together (NULL, 0: none yet)");
    IMCOM_REQUIRE(((uintptr_t)ptr & 255) == 0, "the workspace must be aligned to 256 bytes");
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->aux_stream));
    for (auto s_ : ctx->sub_streams) IMCOM_HIP_CHECK(hipStreamSynchronize(s_));
    if (ctx->ws && !ctx->ws_external) IMCOM_HIP_CHECK(hipFree(ctx->ws));
    ctx->ws = (char *)ptr;
    ctx->ws_bytes = bytes;
    ctx->ws_used = 0;
    ctx->ws_external = true;
    return IMCOM_OK;
}

int imcom_ctx_workspace_needed(imcom_ctx *ctx, size_t *bytes)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(bytes, "null bytes");
    *bytes = ctx->ws_need;
    return IMCOM_OK;
}

int imcom_ctx_set_repair_hint(imcom_ctx *ctx, double lmin_abs)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(lmin_abs >= 0.0 && std::isfinite(lmin_abs), "repair hint: a finite |lambda_min| >= 0 (0 clears it)");
    ctx->repair_hint = lmin_abs;
    return IMCOM_OK;
}

int imcom_ctx_set_repair_expect(imcom_ctx *ctx, int expect)
{
    IMCOM_TRY(enter(ctx));
    ctx->repair_expect = expect != 0;
    return IMCOM_OK;
}

int imcom_ctx_last_repair(imcom_ctx *ctx, int *count, double *w0_min, double *w0_max)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count && w0_min && w0_max, "null output");
    *count = ctx->last_repair_count;
    *w0_min = ctx->last_repair_count ? ctx->last_w0_min : 0.0;
    *w0_max = ctx->last_repair_count ? ctx->last_w0_max : 0.0;
    return IMCOM_OK;
}

// Bytes of workspace imcom_solve_chol_resident (and _begin / _redo) takes: pure arithmetic, for a planner
int imcom_solve_chol_workspace(int batch, int ldn, int m, int ldm, int nv, size_t *bytes)
{
    IMCOM_REQUIRE(batch >= 1 && ldn >= NB && ldn % NB == 0 && ldm >= NB && ldm % NB == 0 && m >= 1 && m <= ldm && nv >= 1 && nv <= CHOL_MAXNV && bytes,
                  "bad sizes (ldn, ldm multiples of 128)");
    *bytes = chol_core_bytes(batch, ldn, m, ldm, nv);
    return IMCOM_OK;
}

int imcom_ctx_profile_enable(imcom_ctx *ctx, int on)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(profile_collect(ctx));
    ctx->profile = on != 0;
    ctx->profile_fine = on >= 2;
    return IMCOM_OK;
}

int imcom_ctx_profile_reset(imcom_ctx *ctx)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(profile_collect(ctx));
    ctx->prof.clear();
    return IMCOM_OK;
}

int imcom_ctx_profile_get(imcom_ctx *ctx, const char *family, double *ms, long *launches)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(family && ms && launches, "null argument");
    IMCOM_TRY(profile_collect(ctx));
    auto it = ctx->prof.find(family);
    *ms = it == ctx->prof.end() ? 0.0 : it->second.ms;
    *launches = it == ctx->prof.end() ? 0 : it->second.launches;
    return IMCOM_OK;
}

int imcom_ctx_mfma_probe(imcom_ctx *ctx, double millis, double *tflops)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(tflops && millis > 0.0 && millis <= 5000.0, "bad arguments (millis in (0, 5000])");
    const int nwg = 2 * ctx->cu_count;  // two 8-wave workgroups per CU: four waves per SIMD, all resident at once
    IMCOM_TRY(ws_reserve(ctx, 4096));
    double *sink;
    IMCOM_TRY(ws_take(ctx, 1, &sink, "imcom_ctx_mfma_probe"));
    hipEvent_t e0, e1;
    IMCOM_HIP_CHECK(hipEventCreate(&e0));
    IMCOM_HIP_CHECK(hipEventCreate(&e1));
    int iters = 200, waves = 8;  // calibrated on a short first run
    double ms = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        IMCOM_HIP_CHECK(hipEventRecord(e0, ctx->stream));
        IMCOM_TRY(launch_mfma_probe(ctx, nwg, iters, sink, &waves));
        IMCOM_HIP_CHECK(hipEventRecord(e1, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        float f = 0.f;
        IMCOM_HIP_CHECK(hipEventElapsedTime(&f, e0, e1));
        ms = f;
        if (pass == 0) iters = (int)std::max(200.0, std::min(2.0e7, iters * millis / std::max(ms, 1e-3)));
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *tflops = (double)nwg * waves * 8.0 * iters * 2048.0 / (ms * 1e-3) / 1e12;  // 16 x 16 x 4 x 2 flop per MFMA and wave
    return IMCOM_OK;
}

int imcom_ctx_gemm_probe(imcom_ctx *ctx, int variant, int M, int N, int K, int batch, int reps, double *tflops)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(variant == 0 || (variant >= 2 && variant <= 4), "gemm probe variant %d: 0, 2, 3 or 4", variant);
    IMCOM_REQUIRE(tflops && M >= 256 && N >= 128 && K >= 16 && batch >= 1 && reps >= 1, "bad arguments");
    IMCOM_REQUIRE(M % 256 == 0 && N % 128 == 0 && K % 16 == 0, "gemm probe: M % 256, N % 128, K % 16");
    const size_t a = (size_t)batch * M * K * 8, b = (size_t)batch * K * N * 8, c = (size_t)batch * M * N * 8;
    IMCOM_TRY(ws_reserve(ctx, a + b + c + 4096));
    double *A = (double *)ws_take(ctx, a), *B = (double *)ws_take(ctx, b), *C = (double *)ws_take(ctx, c);
    if (!A || !B || !C) return ws_short("imcom_ctx_gemm_probe");
    IMCOM_TRY(launch_probe_fill(ctx, A, (long)(a / 8), 1u));  // pseudo-random operands: the power (and clock) of real data
    IMCOM_TRY(launch_probe_fill(ctx, B, (long)(b / 8), 2u));
    hipEvent_t e0, e1;
    IMCOM_HIP_CHECK(hipEventCreate(&e0));
    IMCOM_HIP_CHECK(hipEventCreate(&e1));
    auto run = [&]() -> int {
        // variants 2-4: the engine's other operand layouts (2: both row-major, the Cholesky updates' form C = A B^T; 3: both k-major,
        // the backward solves'; 4: A k-major, B row-major) on the same buffers
        if (variant == 2) return launch_gemm(ctx, false, false, M, N, K, batch, A, K, (long)M * K, B, K, (long)K * N, C, N, (long)M * N, 1.0, 0.0);
        if (variant == 3) return launch_gemm(ctx, true, true, M, N, K, batch, A, M, (long)M * K, B, N, (long)K * N, C, N, (long)M * N, 1.0, 0.0);
        if (variant == 4) return launch_gemm(ctx, true, false, M, N, K, batch, A, M, (long)M * K, B, K, (long)K * N, C, N, (long)M * N, 1.0, 0.0);
        return launch_gemm(ctx, false, true, M, N, K, batch, A, K, (long)M * K, B, N, (long)K * N, C, N, (long)M * N, 1.0, 0.0);
    };
    IMCOM_TRY(run());  // warm-up
    IMCOM_HIP_CHECK(hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; r++) IMCOM_TRY(run());
    IMCOM_HIP_CHECK(hipEventRecord(e1, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    IMCOM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *tflops = 2.0 * M * N * K * batch * reps / (ms * 1e-3) / 1e12;
    return IMCOM_OK;
}

// ---------------------------------------------------------------------------------------------
// native-routine seam: host pointers are staged through the workspace; device pointers used as is (Stage).
int imcom_d5512_getw(imcom_ctx *ctx, const double *fh, long n, double *w, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(n >= 0 && (n == 0 || (fh && w)), "bad arguments");
    if (n == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * 8, (size_t)n * 10 * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *fh_d;
    double *w_d;
    IMCOM_TRY(st.in(fh, n, &fh_d));
    IMCOM_TRY(st.inout(w, (size_t)n * 10, &w_d));
    IMCOM_TRY(launch_getw(ctx, fh_d, n, w_d));
    IMCOM_TRY(st.back(w, w_d, (size_t)n * 10));
    return st.done();
}

int imcom_interp_d5512(imcom_ctx *ctx, const double *infunc, int nlayer, int ngy, int ngx, const double *xpos,
                       const double *ypos, long nout, double *fhatout, int sym, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(infunc && xpos && ypos && fhatout, "null pointer");
    IMCOM_REQUIRE(nlayer >= 1 && ngy >= 1 && ngx >= 1 && nout >= 0, "bad sizes");
    if (sym) {
        long sq = (long)sqrt((double)(nout + 1));
        IMCOM_REQUIRE(sq * sq <= nout, "iD5512C_sym: nout=%ld smaller than its square side^2", nout);
    }
    Stage st(ctx, memspace, __func__);
    const size_t ntab = (size_t)nlayer * ngy * ngx, no = (size_t)nlayer * nout;
    WsPlan plan;
    st.plan(plan, {ntab * 8, (size_t)nout * 8, (size_t)nout * 8, no * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *f_d, *x_d, *y_d;
    double *o_d;
    IMCOM_TRY(st.in(infunc, ntab, &f_d));
    IMCOM_TRY(st.in(xpos, nout, &x_d));
    IMCOM_TRY(st.in(ypos, nout, &y_d));
    IMCOM_TRY(st.inout(fhatout, no, &o_d));  // in-place semantics: untouched elements keep their values
    { ProfScope ps(ctx, "interp"); IMCOM_TRY(launch_interp(ctx, f_d, nlayer, ngy, ngx, x_d, y_d, nout, o_d, sym)); }
    IMCOM_TRY(st.back(fhatout, o_d, no));
    return st.done();
}

int imcom_grid_d5512(imcom_ctx *ctx, const double *infunc, int ngy, int ngx, const double *xpos, const double *ypos,
                     long npi, int nxo, int nyo, double *fhatout, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(infunc && xpos && ypos && fhatout, "null pointer");
    IMCOM_REQUIRE(ngy >= 10 && ngx >= 10 && npi >= 0 && nxo >= 1 && nyo >= 1, "bad sizes");
    Stage st(ctx, memspace, __func__);
    const size_t ntab = (size_t)ngy * ngx, no = (size_t)npi * nxo * nyo;
    WsPlan plan;
    st.plan(plan, {ntab * 8, (size_t)npi * nxo * 8, (size_t)npi * nyo * 8, no * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *f_d, *x_d, *y_d;
    double *o_d;
    IMCOM_TRY(st.in(infunc, ntab, &f_d));
    IMCOM_TRY(st.in(xpos, (size_t)npi * nxo, &x_d));
    IMCOM_TRY(st.in(ypos, (size_t)npi * nyo, &y_d));
    IMCOM_TRY(st.out(fhatout, no, &o_d));
    { ProfScope ps(ctx, "interp"); IMCOM_TRY(launch_grid(ctx, f_d, ngy, ngx, x_d, y_d, npi, nxo, nyo, o_d)); }
    IMCOM_TRY(st.back(fhatout, o_d, no));
    return st.done();
}

int imcom_lakernel1(imcom_ctx *ctx, const double *lam, const double *mPhalf, long m, long n, double C, double targetleak,
                    double kCmin, double kCmax, int nbis, double *kappa, double *Sigma, double *UC, double *T, double smax,
                    int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(lam && mPhalf && kappa && Sigma && UC && T, "null pointer");
    IMCOM_REQUIRE(m >= 0 && n >= 0 && nbis >= 0, "bad sizes");
    Stage st(ctx, memspace, __func__);
    const size_t mn = (size_t)m * n;
    WsPlan plan;
    st.plan(plan, {(size_t)n * 8, mn * 8, (size_t)m * 8, (size_t)m * 8, (size_t)m * 8, mn * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *lam_d, *p_d;
    double *k_d, *S_d, *U_d, *T_d;
    IMCOM_TRY(st.in(lam, n, &lam_d));
    IMCOM_TRY(st.in(mPhalf, mn, &p_d));
    IMCOM_TRY(st.out(kappa, m, &k_d));
    IMCOM_TRY(st.out(Sigma, m, &S_d));
    IMCOM_TRY(st.out(UC, m, &U_d));
    IMCOM_TRY(st.out(T, mn, &T_d));
    { ProfScope ps(ctx, "lakernel1"); IMCOM_TRY(launch_lakernel1(ctx, lam_d, p_d, m, n, n, C, targetleak, kCmin, kCmax, nbis, k_d, S_d, U_d, T_d, n, smax)); }
    IMCOM_TRY(st.back(kappa, k_d, m));
    IMCOM_TRY(st.back(Sigma, S_d, m));
    IMCOM_TRY(st.back(UC, U_d, m));
    IMCOM_TRY(st.back(T, T_d, mn));
    return st.done();
}

int imcom_build_reduced_T(imcom_ctx *ctx, const double *Nflat, const double *Dflat, const double *Eflat, const double *kappa,
                          int nv, long m, double ucmin, double smax, double *out_kappa, double *out_Sigma, double *out_UC,
                          double *out_w, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(Nflat && Dflat && Eflat && kappa && out_kappa && out_Sigma && out_UC && out_w, "null pointer");
    IMCOM_REQUIRE(m >= 0 && nv >= 2, "bad sizes (nv must be >= 2, routine.py:537)");
    Stage st(ctx, memspace, __func__);
    const size_t nv2 = (size_t)nv * nv, mv = (size_t)m * nv;
    WsPlan plan;
    st.plan(plan, {(size_t)m * nv2 * 8, mv * 8, (size_t)m * nv2 * 8, (size_t)nv * 8, (size_t)m * 8, (size_t)m * 8, (size_t)m * 8, mv * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *N_d, *D_d, *E_d, *k_d;
    double *ok, *oS, *oU, *ow;
    IMCOM_TRY(st.in(Nflat, (size_t)m * nv2, &N_d));
    IMCOM_TRY(st.in(Dflat, mv, &D_d));
    IMCOM_TRY(st.in(Eflat, (size_t)m * nv2, &E_d));
    IMCOM_TRY(st.in(kappa, nv, &k_d));
    IMCOM_TRY(st.out(out_kappa, m, &ok));
    IMCOM_TRY(st.out(out_Sigma, m, &oS));
    IMCOM_TRY(st.out(out_UC, m, &oU));
    IMCOM_TRY(st.out(out_w, mv, &ow));
    { ProfScope ps(ctx, "reduced_T"); IMCOM_TRY(launch_build_reduced_T(ctx, N_d, D_d, E_d, k_d, nv, m, ucmin, smax, ok, oS, oU, ow)); }
    IMCOM_TRY(st.back(out_kappa, ok, m));
    IMCOM_TRY(st.back(out_Sigma, oS, m));
    IMCOM_TRY(st.back(out_UC, oU, m));
    IMCOM_TRY(st.back(out_w, ow, mv));
    return st.done();
}

// ---------------------------------------------------------------------------------------------
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

// ---------------------------------------------------------------------------------------------
int imcom_build_A(imcom_ctx *ctx, int batch, const int *n_host, int ldn, const double *x, const double *y, const int *psf,
                  const double *tables, int ntab, const imcom_table_geom *geom, const int *pair_tab, const double *pair_pen,
                  int npsf_max, double *A)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && n_host && x && y && psf && tables && geom && pair_tab && pair_pen && A, "null pointer");
    IMCOM_REQUIRE(ldn >= 1 && ntab >= 1 && npsf_max >= 1 && geom->nsamp >= 1 && geom->dscale > 0, "bad sizes");
    const long nt_ = (ldn + 15) / 16, tiles_ = nt_ * (nt_ + 1) / 2 * batch;  // per-stamp tile order by PSF pair: key + descriptor per tile, bins per stamp
    IMCOM_TRY(ws_reserve(ctx, (size_t)batch * 4 + (size_t)tiles_ * 8 + (size_t)batch * ((size_t)npsf_max * npsf_max + 1) * 4 + 8192));
    int *n_dev = (int *)ws_take(ctx, (size_t)batch * 4);
    IMCOM_TRY(upload(ctx, n_dev, n_host, batch));
    ProfScope ps(ctx, "build_A");
    return launch_build_A(ctx, batch, n_dev, ldn, x, y, psf, tables, ntab, geom->nsamp + 12, geom->nc, geom->dscale, pair_tab,
                          pair_pen, npsf_max, A);
}

int imcom_build_B(imcom_ctx *ctx, int batch, const int *n_host, int ldn, const double *x, const double *y, const int *psf,
                  const double *tables, int ntab, const imcom_table_geom *geom, const int *io_tab, int npsf_max,
                  const double *out_x0, const double *out_y0, int n2f, int ldm, double *Bt)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && n_host && x && y && psf && tables && geom && io_tab && out_x0 && out_y0 && Bt, "null pointer");
    IMCOM_REQUIRE(ldn >= 1 && ntab >= 1 && npsf_max >= 1 && n2f >= 1 && ldm >= n2f * n2f, "bad sizes");
    IMCOM_TRY(ws_reserve(ctx, (size_t)batch * 4 + 1024));
    int *n_dev = (int *)ws_take(ctx, (size_t)batch * 4);
    IMCOM_TRY(upload(ctx, n_dev, n_host, batch));
    ProfScope ps(ctx, "build_B");
    return launch_build_B(ctx, batch, n_dev, ldn, x, y, psf, tables, geom->nsamp + 12, geom->nc, geom->dscale, io_tab,
                          npsf_max, out_x0, out_y0, n2f, ldm, Bt);
}

int imcom_coadd_epilogue(imcom_ctx *ctx, int batch, const int *n_host, int ldn, int m, int ldm, int n2f, int fade, int n2,
                         float *Tt, const float *indata, int n_inframe, const int *expo, int n_expo, float *outimage,
                         double *Tsum_stamp, double *Tsum_inpix, double *Neff)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && n_host && Tt && indata && expo && outimage && Tsum_stamp && Tsum_inpix && Neff, "null pointer");
    IMCOM_REQUIRE(m == n2f * n2f && m <= ldm && n_inframe >= 1 && n_expo >= 1 && fade >= 0 && n2 >= 1, "bad sizes");
    IMCOM_TRY(ws_reserve(ctx, (size_t)batch * 4 + (size_t)batch * m * n_expo * 8 + 2048));
    int *n_dev = (int *)ws_take(ctx, (size_t)batch * 4);
    double *Tsum_image = (double *)ws_take(ctx, (size_t)batch * m * n_expo * 8);
    IMCOM_TRY(upload(ctx, n_dev, n_host, batch));
    ProfScope ps(ctx, "epilogue");
    return launch_epilogue(ctx, batch, n_dev, ldn, m, ldm, n2f, fade, n2, Tt, indata, n_inframe, expo, n_expo, outimage,
                           Tsum_image, Tsum_stamp, Tsum_inpix, Neff);
}

int imcom_trapezoid_f32(imcom_ctx *ctx, float *maps, long nmaps, int n2f, int fade)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(maps && nmaps >= 0 && n2f >= 1 && fade >= 0, "bad arguments");
    return launch_trapezoid_f32(ctx, maps, nmaps, n2f, fade);
}

int imcom_clamp_min_f32(imcom_ctx *ctx, float *maps, long count, float lo)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && (count == 0 || maps), "bad arguments");
    return launch_clamp_min_f32(ctx, maps, count, lo);
}

// ---------------------------------------------------------------------------------------------
// injected star layers (inject.hip)
int imcom_psf_from_cube(imcom_ctx *ctx, int na, const double *cube, int ny, int nx, int nstar, const double *lpoly, double tophatwidth,
                        double gaussiansigma, double scale, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(na >= 1 && cube && ny >= 1 && nx >= 1 && nstar >= 0 && (nstar == 0 || (lpoly && out)), "bad arguments");
    IMCOM_REQUIRE(tophatwidth >= 0.0 && gaussiansigma >= 0.0 && tophatwidth + 6.0 * gaussiansigma < 4096.0 && scale == scale,
                  "bad smearing widths or scale");
    if (nstar == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    const int npad = imcom_smooth_pad_width(tophatwidth, gaussiansigma), nyy = ny + 2 * npad, nxx = nx + 2 * npad;
    const size_t szCube = (size_t)na * ny * nx, szL = (size_t)nstar * na, npix = (size_t)nyy * nxx, szOut = (size_t)nstar * npix;
    WsPlan plan;
    plan.add(smooth_pad_ws_bytes(na, ny, nx, tophatwidth, gaussiansigma));
    plan.add((size_t)na * npix * 8);
    st.plan(plan, {szCube * 8, szL * 8, szOut * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    SmoothPadWs w;
    IMCOM_TRY(smooth_pad_take(ctx, na, ny, nx, tophatwidth, gaussiansigma, &w, __func__));
    double *planes, *out_d;
    IMCOM_TRY(ws_take(ctx, (size_t)na * npix, &planes, __func__));
    const double *cube_d, *lpoly_d;
    IMCOM_TRY(st.in(cube, szCube, &cube_d));
    IMCOM_TRY(st.in(lpoly, szL, &lpoly_d));
    IMCOM_TRY(st.out(out, szOut, &out_d));
    IMCOM_TRY(smooth_pad_device(ctx, w, na, cube_d, ny, nx, tophatwidth, gaussiansigma, planes));
    IMCOM_TRY(launch_cube_contract(ctx, planes, na, (long)npix, lpoly_d, nstar, scale, out_d));
    IMCOM_TRY(st.back(out, out_d, szOut));
    return st.done();
}

int imcom_draw_stars(imcom_ctx *ctx, int nstar, const double *psfs, int py, int px, const double *xsca, const double *ysca, double oversamp,
                     int d, int nside, double *image, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(nstar >= 0 && image && (nstar == 0 || (psfs && xsca && ysca)), "null pointer");
    IMCOM_REQUIRE(py >= 1 && px >= 1 && py <= 16384 && px <= 16384 && d >= 1 && d <= 65536 && nside >= 1 && nside <= 65536, "bad sizes");
    IMCOM_REQUIRE(oversamp >= 1.0e-3 && oversamp <= 1.0e6, "oversamp %g out of range", oversamp);
    if (nstar == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    const size_t szP = (size_t)nstar * py * px, szI = (size_t)nside * nside;
    WsPlan plan;
    st.plan(plan, {szP * 8, (size_t)nstar * 8, (size_t)nstar * 8, szI * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *p_d, *x_d, *y_d;
    double *img_d;
    IMCOM_TRY(st.in(psfs, szP, &p_d));
    IMCOM_TRY(st.in(xsca, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(ysca, (size_t)nstar, &y_d));
    IMCOM_TRY(st.inout(image, szI, &img_d));  // the stars are added to what the image holds
    IMCOM_TRY(launch_draw_stars(ctx, nstar, p_d, py, px, x_d, y_d, oversamp, d, nside, img_d));
    IMCOM_TRY(st.back(image, img_d, szI));
    return st.done();
}

// ---------------------------------------------------------------------------------------------
// the long-range PSF part of an SCA image (imsubtract.hip)
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

// ---------------------------------------------------------------------------------------------
// the split of a PSF cube into its short- and long-range parts (splitpsf.hip)
static int splitpsf_lorder1(int npoly)
{
    int l1 = 1;
    while (l1 * l1 < npoly) l1++;
    return l1 * l1 == npoly ? l1 : 0;
}

int imcom_splitpsf_sizes(int n, int npoly, double width, int nsca, int npts, long *out)
{
    IMCOM_REQUIRE(out, "null out");
    IMCOM_REQUIRE(n >= 2 && n <= 65536 && npoly >= 1 && npoly <= 4096 && nsca >= 1 && npts >= 1 && npts <= npoly && width > 0.0 && width <= 4096.0,
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
    IMCOM_REQUIRE(nplane >= 1 && nplane <= 65535 && n >= 1 && n <= SPLITPSF_MAXN && width > 0.0 && width <= 4096.0, "splitpsf tophat: %d planes of side %d, width %g",
                  nplane, n, width);
    if (!splitpsf_route(n + 2 * splitpsf_tophat_npad(width))) {
        set_error("splitpsf tophat: a padded side of %d is beyond the %d this build transforms", n + 2 * splitpsf_tophat_npad(width), SPLITPSF_MAXN);
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
    IMCOM_REQUIRE(npoly >= 1 && n >= 2 && n <= SPLITPSF_MAXN && n % 2 == 0 && ns >= 2 && ns <= n && ns % 2 == 0, "SplitPSF requires even dimension (%d, %d)", n, ns);
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
        set_error("splitpsf: a cube side of %d needs transforms of %d, beyond the %d this build transforms", n, 2 * n, SPLITPSF_MAXN);
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

// ---------------------------------------------------------------------------------------------
// destriping: cost and gradient over a resident mosaic (destripe.hip)
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
                         int *max_np)
{
    IMCOM_REQUIRE(npairs >= 0 && (npairs == 0 || (pa && pb && px && py && pl)), "destripe: null pair table");
    int run = 0;
    *max_np = 0;
    for (int i = 0; i < npairs; i++) {
        IMCOM_REQUIRE(pa[i] >= 0 && pa[i] < n_sca && pb[i] >= 0 && pb[i] < n_sca && pa[i] != pb[i], "destripe: pair %d is (%d, %d) of %d SCAs", i, pa[i], pb[i], n_sca);
        IMCOM_REQUIRE(i == 0 || pa[i] > pa[i - 1] || (pa[i] == pa[i - 1] && pb[i] > pb[i - 1]), "destripe: the pair table is not sorted by (a, b) at %d", i);
        IMCOM_REQUIRE((px[i] && py[i]) || (!px[i] && !py[i] && pl[i] && L >= 2), "destripe: pair %d has neither position arrays nor a lattice", i);
        run = (i > 0 && pa[i] == pa[i - 1]) ? run + 1 : 1;
        if (run > *max_np) *max_np = run;
    }
    return IMCOM_OK;
}

int destripe_upload_pairs(imcom_ctx *ctx, int n_sca, int npairs, const int *pa, const int *pb, const void *const *px, const void *const *py,
                          const void *const *pl, DsPair **pairs_d, int **start_d, const char *who)
{
    std::vector<DsPair> tab((size_t)std::max(npairs, 1));
    std::vector<int> start((size_t)n_sca + 1, 0);
    for (int i = 0; i < npairs; i++) {
        tab[i].x = (const double *)px[i], tab[i].y = (const double *)py[i], tab[i].lat = (const double *)pl[i], tab[i].a = pa[i], tab[i].b = pb[i];
        start[pa[i] + 1]++;
    }
    for (int a = 0; a < n_sca; a++) start[a + 1] += start[a];
    IMCOM_TRY(ws_take(ctx, tab.size(), pairs_d, who));
    IMCOM_TRY(ws_take(ctx, start.size(), start_d, who));
    IMCOM_TRY(upload(ctx, *pairs_d, tab.data(), tab.size()));
    return upload(ctx, *start_d, start.data(), start.size());
}

size_t destripe_cost_ws(const DsGeom &g, int npairs, bool forward)
{
    WsPlan plan;
    plan.add((size_t)std::max(npairs, 1) * sizeof(DsPair));
    plan.add(((size_t)g.n_sca + 1) * sizeof(int));
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
    plan.add((size_t)g.n_sca * g.nbins * 8);
    plan.add((size_t)g.n_sca * g.nside * std::max(g.ncb, 1) * 8);
    plan.add(8);
    plan.add(16);
    plan.add((size_t)g.n_sca * g.nbins * 8);
    return plan.total;
}
}  // namespace

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
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, double *neff)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(mask && neff && (L == 0 || W), "null pointer");
    int max_np;
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &max_np));
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, nside, 0, L, max_np, &g));
    IMCOM_TRY(ws_reserve(ctx, destripe_cost_ws(g, npairs, false)));
    DsPair *pairs_d;
    int *start_d;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &pairs_d, &start_d, __func__));
    return launch_destripe_forward(ctx, g, true, nullptr, mask, nullptr, nullptr, pairs_d, start_d, W, neff, nullptr, nullptr);
}

int imcom_destripe_cost(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *image, const unsigned char *mask,
                        const float *geff, const double *neff, const double *params, int npairs, const int *pair_a, const int *pair_b,
                        const void *const *pair_x, const void *const *pair_y, const void *const *pair_lat, const double *W, int model, double thresh,
                        double neff_min, double col_boundary_const, float *psi, double *eps)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && mask && geff && neff && params && psi && eps && (L == 0 || W), "null pointer");
    int max_np;
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &max_np));
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
    double *eps_rows, *pen;
    const int nchunk = (nside + 399) / 400;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &pairs_d, &start_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * nside, &eps_rows, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * std::max(g.ncb - 1, 1) * nchunk, &pen, __func__));
    IMCOM_TRY(launch_destripe_forward(ctx, g, false, image, mask, geff, params, pairs_d, start_d, W, (double *)neff, psi, eps_rows));
    return launch_destripe_eps(ctx, g, image, mask, params, eps_rows, pen, nchunk, eps);
}

int imcom_destripe_residual(imcom_ctx *ctx, int n_sca, int nside, int ds_rows, int amp_cols, int L, const float *psi, const float *geff, const double *neff,
                            int npairs, const int *pair_a, const int *pair_b, const void *const *pair_x, const void *const *pair_y,
                            const void *const *pair_lat, const double *W, int model, double thresh, double geff_max, double *resids, double *resids1,
                            double *resids2)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(psi && geff && neff && resids && (L == 0 || W), "null pointer");
    IMCOM_REQUIRE(geff_max >= 0.0 && geff_max < 1e300, "destripe: geff_max = %g", geff_max);
    int max_np;
    IMCOM_TRY(destripe_check_pairs(n_sca, L, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &max_np));
    DsGeom g;
    IMCOM_TRY(destripe_geom(n_sca, nside, ds_rows, amp_cols, L, max_np, &g));
    IMCOM_TRY(destripe_model(model, thresh, &g));
    IMCOM_TRY(ws_reserve(ctx, destripe_resid_ws(g, npairs)));
    DsPair *pairs_d;
    int *start_d;
    double *term1, *rowcb, *scale;
    unsigned long long *bits, *bins;
    IMCOM_TRY(destripe_upload_pairs(ctx, n_sca, npairs, pair_a, pair_b, pair_x, pair_y, pair_lat, &pairs_d, &start_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * g.nbins, &term1, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * nside * std::max(g.ncb, 1), &rowcb, __func__));
    IMCOM_TRY(ws_take(ctx, 1, &bits, __func__));
    IMCOM_TRY(ws_take(ctx, 2, &scale, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)n_sca * g.nbins, &bins, __func__));
    return launch_destripe_gradient(ctx, g, psi, geff, neff, pairs_d, npairs, W, geff_max, term1, rowcb, bits, scale, bins, resids, resids1, resids2);
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

// ---------------------------------------------------------------------------------------------
// noise power spectra of coadded frames (noisespec.hip)
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
    IMCOM_REQUIRE(L <= SPLITPSF_MAXN, "noise spectra: a side of %d is beyond the %d this build transforms", L, SPLITPSF_MAXN);
    return IMCOM_OK;
}

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
    IMCOM_REQUIRE(nframe >= 1 && nframe <= 65535 && n >= 1 && n <= SPLITPSF_MAXN && nidx >= 1 && nidx <= 65535, "noise spectra: %d frames of side %d, %d annuli", nframe,
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
    IMCOM_REQUIRE(nlayers >= 1 && nlayers <= 65535 && n >= 1 && n <= SPLITPSF_MAXN && nrad >= 1 && bins >= 1 && coverage_bin >= 0 && coverage_bin < bins,
                  "noise spectra: %d layers of side %d, %d annuli, coverage bin %d of %d", nlayers, n, nrad, coverage_bin, bins);
    return launch_noiseps_accumulate(ctx, ps2d, mean, err, nlayers, (long)n * n, nrad, bins, coverage_bin, ps2d_all, ps1d_all);
}

// ---------------------------------------------------------------------------------------------
// PCG64 draws by position and the cosmic-ray mask (pcg64.hip)
namespace {
// the affine maps of 2^j steps of s <- M s + inc, j < PCG64_JUMPS, into the workspace: (A_0, C_0) = (M, inc), A_{j+1} = A_j^2,
// C_{j+1} = (A_j + 1) C_j (mod 2^128)
int pcg64_jumps(imcom_ctx *ctx, uint64_t inc_lo, uint64_t inc_hi, const unsigned long long **jumps_d, const char *who)
{
    typedef unsigned __int128 u128;
    unsigned long long tab[PCG64_JUMPS * 4], *d;
    u128 A = ((u128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull, Cc = ((u128)inc_hi << 64) | inc_lo;
    for (int j = 0; j < PCG64_JUMPS; j++) {
        tab[4 * j] = (unsigned long long)A;
        tab[4 * j + 1] = (unsigned long long)(A >> 64);
        tab[4 * j + 2] = (unsigned long long)Cc;
        tab[4 * j + 3] = (unsigned long long)(Cc >> 64);
        Cc = (A + 1) * Cc;
        A = A * A;
    }
    IMCOM_TRY(ws_take(ctx, (size_t)PCG64_JUMPS * 4, &d, who));
    IMCOM_TRY(upload(ctx, d, tab, (size_t)PCG64_JUMPS * 4));
    *jumps_d = d;
    return IMCOM_OK;
}
constexpr long PCG64_MAX_COUNT = 1L << 36;
}  // namespace

int imcom_pcg64_uniform(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                        long count, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    IMCOM_REQUIRE(count == 0 || out, "null pointer");
    if (count == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {(size_t)count * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi}, offset[2] = {offset_lo, offset_hi};
    double *o_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.out(out, (size_t)count, &o_d));
    IMCOM_TRY(launch_pcg64_uniform(ctx, state, jumps, offset, count, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)count));
    return st.done();
}

int imcom_pcg64_uniform_at(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, const long *pos, long count, double *out,
                           int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    IMCOM_REQUIRE(count == 0 || (pos && out), "null pointer");
    if (count == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {(size_t)count * 8, (size_t)count * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi};
    const long *p_d;
    double *o_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.in(pos, (size_t)count, &p_d));
    IMCOM_TRY(st.out(out, (size_t)count, &o_d));
    IMCOM_TRY(launch_pcg64_uniform_at(ctx, state, jumps, p_d, count, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)count));
    return st.done();
}

int imcom_cr_mask(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, int nside, int pad, int slice, int n_slices,
                  double pcut, const float *labnoise, double threshold, unsigned char *mask, long *ngood, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(mask && ngood, "null pointer");
    IMCOM_REQUIRE(nside >= 1 && nside <= 65536 && pad >= 1 && pad <= 4096, "cr_mask: nside %d outside 1 .. 65536 or pad %d outside 1 .. 4096", nside, pad);
    IMCOM_REQUIRE(n_slices >= 1 && n_slices <= 65536 && slice >= 0 && slice < n_slices, "cr_mask: slice %d of %d", slice, n_slices);
    Stage st(ctx, memspace, __func__);
    const size_t npix = (size_t)nside * nside;
    const unsigned long long W = (unsigned long long)nside + 2ull * pad;  // (slice W^2 + W^2 < 2^16 2^34)
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {labnoise ? npix * 4 : 0, npix, sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi};
    const float *l_d;
    unsigned char *m_d;
    long *n_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.in(labnoise, npix, &l_d));
    IMCOM_TRY(st.out(mask, npix, &m_d));
    IMCOM_TRY(st.out(ngood, (size_t)1, &n_d));
    IMCOM_TRY(launch_cr_mask(ctx, state, jumps, (unsigned long long)slice * W * W, nside, pad, pcut, l_d, threshold, m_d, (unsigned long long *)n_d));
    IMCOM_TRY(st.back(mask, (const unsigned char *)m_d, npix));
    IMCOM_TRY(st.back(ngood, (const long *)n_d, (size_t)1));
    return st.done();
}

// ---------------------------------------------------------------------------------------------
// numpy's normal draws of a PCG64 stream (ziggurat.hip)
namespace {
constexpr int ZIG_TILE_DEFAULT = 1024, ZIG_TILE_MAX = 1024;  // (the LDS of zig_emit_kernel: 36 KB at 1024)
constexpr long ZIG_CHUNK_TILES_DEFAULT = 1L << 16, ZIG_CHUNK_TILES_MAX = 1L << 20;
constexpr double ZIG_GUARD_DEFAULT = ZIG_GUARD;
// the tiles one chunk may need for `remaining` draws: 1.0145 outputs a draw on average, 3 % and a tile allowed for
long zig_tiles_for(long remaining, int P) { return (remaining + remaining / 32 + P - 1) / P + 1; }
}  // namespace

int imcom_pcg64_normal_sizes(long count, long *tail_cap)
{
    IMCOM_REQUIRE(tail_cap, "null pointer");
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    *tail_cap = count / 1024 + 4096;  // the expected number is count / 3700
    return IMCOM_OK;
}

int imcom_pcg64_normal(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                       long count, double *out, long *tail_idx, uint64_t *tail_raw, uint64_t *info, int memspace)
{
    return imcom_pcg64_normal_ex(ctx, state_lo, state_hi, inc_lo, inc_hi, offset_lo, offset_hi, count, out, tail_idx, tail_raw, info, memspace, 0, 0, 0.0);
}

int imcom_pcg64_normal_ex(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                          long count, double *out, long *tail_idx, uint64_t *tail_raw, uint64_t *info, int memspace, int tile, long chunk_tiles, double guard_band)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    IMCOM_REQUIRE(info && (count == 0 || (out && tail_idx && tail_raw)), "null pointer");
    IMCOM_REQUIRE(tile == 0 || (tile >= 4 && tile <= ZIG_TILE_MAX && (tile & (tile - 1)) == 0), "pcg64_normal: tile %d is no power of two in 4 .. %d", tile,
                  ZIG_TILE_MAX);
    IMCOM_REQUIRE(chunk_tiles >= 0 && chunk_tiles <= ZIG_CHUNK_TILES_MAX, "pcg64_normal: %ld tiles a chunk outside 1 .. 2^20", chunk_tiles);
    IMCOM_REQUIRE(guard_band >= 0.0 && guard_band <= 1.0, "pcg64_normal: guard band %g outside 0 .. 1", guard_band);
    for (int i = 0; i < 4; i++) info[i] = 0;
    if (count == 0) return IMCOM_OK;
    const int P = tile ? tile : ZIG_TILE_DEFAULT;
    const long chunk_max = chunk_tiles ? chunk_tiles : ZIG_CHUNK_TILES_DEFAULT;
    const double guard = guard_band > 0.0 ? guard_band : ZIG_GUARD_DEFAULT;
    const long tail_cap = count / 1024 + 4096, tiles_max = std::min(chunk_max, zig_tiles_for(count, P));
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    plan.add((size_t)tiles_max * ZIG_ENTRIES);      // exit_t
    plan.add((size_t)tiles_max * ZIG_ENTRIES * 2);  // count_t
    plan.add((size_t)tiles_max);                    // entry_t
    plan.add((size_t)tiles_max * 8);                // base_t
    plan.add(2 * sizeof(long));                     // res
    plan.add(4 * sizeof(unsigned long long));       // info
    st.plan(plan, {(size_t)count * 8, (size_t)tail_cap * 8, (size_t)tail_cap * 16});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi};
    unsigned char *exit_t, *entry_t;
    unsigned short *count_t;
    long *base_t, *res, *ti_d;
    unsigned long long *info_d, *tr_d;
    double *o_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)tiles_max * ZIG_ENTRIES, &exit_t, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)tiles_max * ZIG_ENTRIES, &count_t, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)tiles_max, &entry_t, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)tiles_max, &base_t, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)2, &res, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)4, &info_d, __func__));
    IMCOM_TRY(st.out(out, (size_t)count, &o_d));
    IMCOM_TRY(st.out(tail_idx, (size_t)tail_cap, &ti_d));
    IMCOM_TRY(st.out((unsigned long long *)tail_raw, (size_t)tail_cap * 2, &tr_d));
    IMCOM_HIP_CHECK(hipMemsetAsync(info_d, 0, 4 * sizeof(unsigned long long), ctx->stream));
    // chunks in ascending order: a chunk's entry offset and output base are the exit of the chunk before
    unsigned long long rel = 0;
    long made = 0, entry = 0;
    while (made < count) {
        const long tiles = std::min(tiles_max, zig_tiles_for(count - made, P));
        const unsigned long long lo = offset_lo + rel, start[2] = {lo, offset_hi + (lo < rel)};
        long res_h[2];
        IMCOM_TRY(launch_zig_chunk(ctx, state, jumps, start, rel, P, tiles, (int)entry, made, guard, exit_t, count_t, entry_t, base_t, res, count, o_d, ti_d,
                                   tr_d, tail_cap, info_d));
        IMCOM_HIP_CHECK(hipMemcpyAsync(res_h, res, sizeof(res_h), hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        entry = res_h[0];
        made = res_h[1];
        rel += (unsigned long long)tiles * P;
    }
    unsigned long long info_h[4];
    IMCOM_HIP_CHECK(hipMemcpyAsync(info_h, info_d, sizeof(info_h), hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const long tails = (long)std::min<unsigned long long>(info_h[2], (unsigned long long)tail_cap);
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)count));
    IMCOM_TRY(st.back(tail_idx, (const long *)ti_d, (size_t)tails));
    IMCOM_TRY(st.back((unsigned long long *)tail_raw, (const unsigned long long *)tr_d, (size_t)tails * 2));
    info[0] = info_h[0];
    info[1] = info_h[1];
    info[2] = info_h[2];
    info[3] = info_h[3] != 0;
    return st.done();
}

// ---------------------------------------------------------------------------------------------
// The transform of the 1/f noise layer (noise1f.hip)
int imcom_noise_1f(imcom_ctx *ctx, const double *normals, const double *amp, long len, int nch, int w, int border, float *frame, double *block, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(len >= 2 && nch >= 1 && nch <= 4096 && w >= 1 && border >= 0, "noise_1f: len %ld, %d channels of width %d, border %d", len, nch, w, border);
    int N1, N2;
    if ((w & (w - 1)) || !noise1f_split(len, &N1, &N2) || (long)w > len / 2) {
        set_error("noise_1f: the length (%ld) must be a power of two in 2^10 .. 2^20 and the channel width (%d) a power of two up to half of it", len, w);
        return IMCOM_ERR_UNSUPPORTED;
    }
    IMCOM_REQUIRE(normals && amp && frame, "null pointer");
    const long half = len / 2, rows = half / w, cols = (long)nch * w;
    IMCOM_REQUIRE(2L * border < rows && 2L * border < cols, "noise_1f: a border of %d leaves nothing of %ld x %ld pixels", border, rows, cols);
    const long npix = (rows - 2 * border) * (cols - 2 * border);
    const int group = std::min(nch, NOISE1F_GROUP);
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)N1 * 16);
    plan.add((size_t)N2 * 16);
    plan.add((size_t)group * len * 16);  // S
    plan.add((size_t)nch * 8);           // sums
    if (st.host || !block) plan.add((size_t)nch * half * 8);
    st.plan(plan, {(size_t)2 * nch * len * 8, (size_t)len * 8, (size_t)npix * 4});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    double2 *tw1, *tw2, *S;
    double *sum, *blk = block;
    const double *g_d, *amp_d;
    float *f_d;
    IMCOM_TRY(ws_take(ctx, (size_t)N1, &tw1, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)N2, &tw2, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)group * len, &S, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)nch, &sum, __func__));
    if (st.host || !block) IMCOM_TRY(ws_take(ctx, (size_t)nch * half, &blk, __func__));
    IMCOM_TRY(st.in(normals, (size_t)2 * nch * len, &g_d));
    IMCOM_TRY(st.in(amp, (size_t)len, &amp_d));
    IMCOM_TRY(st.out(frame, (size_t)npix, &f_d));
    IMCOM_TRY(noise1f_tables(ctx, len, tw1, tw2));
    for (int ch0 = 0; ch0 < nch; ch0 += group)
        IMCOM_TRY(launch_noise1f_group(ctx, g_d, amp_d, len, ch0, std::min(group, nch - ch0), tw1, tw2, S, blk));
    IMCOM_TRY(launch_noise1f_place(ctx, blk, sum, len, nch, w, border, f_d));
    IMCOM_TRY(st.back(frame, (const float *)f_d, (size_t)npix));
    if (block) IMCOM_TRY(st.back(block, (const double *)blk, (size_t)nch * half));
    return st.done();
}

// ---------------------------------------------------------------------------------------------
// Bright-object masks of the destripe set-up (objmask.hip)
namespace {
constexpr long MASK_MAX_SIDE = 65536;
}

int imcom_select_kth(imcom_ctx *ctx, const void *values, int is_f64, long n, const unsigned char *flags, int use_abs, double c, long k, void *out, long *info,
                     int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(values && out && info, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "select_kth: n = %ld outside 1 .. 2^32", n);
    IMCOM_REQUIRE(k < n, "select_kth: rank %ld of %ld values", k, n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add(SELECT_STATE * sizeof(unsigned long long));
    plan.add(2 * SELECT_BINS * sizeof(unsigned long long));
    st.plan(plan, {(size_t)n * esz, flags ? (size_t)n : 0, 2 * esz, 2 * sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *state, *hist;
    const char *v_d;
    const unsigned char *f_d;
    char *o_d;
    long *i_d;
    IMCOM_TRY(ws_take(ctx, (size_t)SELECT_STATE, &state, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)2 * SELECT_BINS, &hist, __func__));
    IMCOM_TRY(st.in((const char *)values, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.in(flags, (size_t)n, &f_d));
    IMCOM_TRY(st.out((char *)out, 2 * esz, &o_d));
    IMCOM_TRY(st.out(info, (size_t)2, &i_d));
    IMCOM_TRY(launch_select_kth(ctx, v_d, is_f64 != 0, f_d, n, use_abs != 0, c, k, state, hist, o_d, i_d));
    IMCOM_TRY(st.back((char *)out, (const char *)o_d, 2 * esz));
    IMCOM_TRY(st.back(info, (const long *)i_d, (size_t)2));
    return st.done();
}

int imcom_mask_threshold(imcom_ctx *ctx, const void *image, int is_f64, long n, double bkg, double t_seed, double t_grow, int finite_only, unsigned char *seed,
                         unsigned char *grow, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && seed, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_threshold: n = %ld outside 1 .. 2^32", n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, (size_t)n, grow ? (size_t)n : 0});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d;
    unsigned char *s_d, *g_d = nullptr;
    IMCOM_TRY(st.in((const char *)image, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.out(seed, (size_t)n, &s_d));
    if (grow) IMCOM_TRY(st.out(grow, (size_t)n, &g_d));
    IMCOM_TRY(launch_mask_threshold(ctx, v_d, is_f64 != 0, n, bkg, t_seed, t_grow, finite_only != 0, s_d, g_d));
    IMCOM_TRY(st.back(seed, (const unsigned char *)s_d, (size_t)n));
    if (grow) IMCOM_TRY(st.back(grow, (const unsigned char *)g_d, (size_t)n));
    return st.done();
}

int imcom_mask_clip(imcom_ctx *ctx, const void *image, int is_f64, long n, const unsigned char *keep_in, double bkg, double t, unsigned char *keep_out, long *count,
                    int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(image && keep_out && count, "null pointer");
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_clip: n = %ld outside 1 .. 2^32", n);
    const size_t esz = is_f64 ? 8 : 4;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, keep_in ? (size_t)n : 0, (size_t)n, sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d;
    const unsigned char *ki_d;
    unsigned char *ko_d;
    long *c_d;
    IMCOM_TRY(st.in((const char *)image, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.in(keep_in, (size_t)n, &ki_d));
    IMCOM_TRY(st.out(keep_out, (size_t)n, &ko_d));
    IMCOM_TRY(st.out(count, (size_t)1, &c_d));
    IMCOM_TRY(launch_mask_clip(ctx, v_d, is_f64 != 0, n, ki_d, bkg, t, ko_d, (unsigned long long *)c_d));
    IMCOM_TRY(st.back(keep_out, (const unsigned char *)ko_d, (size_t)n));
    IMCOM_TRY(st.back(count, (const long *)c_d, (size_t)1));
    return st.done();
}

int imcom_mask_propagate(imcom_ctx *ctx, const unsigned char *seed, const unsigned char *grow, int rows, int cols, unsigned char *out, long *sweeps, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(seed && grow && out, "null pointer");
    IMCOM_REQUIRE(rows >= 1 && rows <= MASK_MAX_SIDE && cols >= 1 && cols <= MASK_MAX_SIDE, "mask_propagate: %d x %d pixels, sides 1 .. 65536", rows, cols);
    IMCOM_REQUIRE(out != grow, "mask_propagate: the result cannot overwrite the grow image");
    const size_t npix = (size_t)rows * cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add(npix);
    plan.add(sizeof(unsigned int));
    st.plan(plan, {npix, npix, npix});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned char *tmp, *o_d;
    unsigned int *changed;
    const unsigned char *s_d, *g_d;
    IMCOM_TRY(ws_take(ctx, npix, &tmp, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)1, &changed, __func__));
    IMCOM_TRY(st.in(seed, npix, &s_d));
    IMCOM_TRY(st.in(grow, npix, &g_d));
    IMCOM_TRY(st.out(out, npix, &o_d));
    if (o_d != s_d) IMCOM_HIP_CHECK(hipMemcpyAsync(o_d, s_d, npix, hipMemcpyDeviceToDevice, ctx->stream));
    long n_sweeps = 0;
    IMCOM_TRY(launch_mask_propagate(ctx, g_d, rows, cols, o_d, tmp, changed, &n_sweeps));
    if (sweeps) *sweeps = n_sweeps;
    IMCOM_TRY(st.back(out, (const unsigned char *)o_d, npix));
    return st.done();
}

int imcom_mask_dilate(imcom_ctx *ctx, const unsigned char *in, int rows, int cols, int r, unsigned char *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(in && out, "null pointer");
    IMCOM_REQUIRE(rows >= 1 && rows <= MASK_MAX_SIDE && cols >= 1 && cols <= MASK_MAX_SIDE, "mask_dilate: %d x %d pixels, sides 1 .. 65536", rows, cols);
    IMCOM_REQUIRE(in != out, "mask_dilate: not in place");
    if (r < 1 || r > MASK_DILATE_MAX_R) {
        set_error("mask_dilate: radius %d, served are 1 .. %d", r, MASK_DILATE_MAX_R);
        return IMCOM_ERR_UNSUPPORTED;
    }
    const size_t npix = (size_t)rows * cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {npix, npix});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned char *i_d;
    unsigned char *o_d;
    IMCOM_TRY(st.in(in, npix, &i_d));
    IMCOM_TRY(st.out(out, npix, &o_d));
    IMCOM_TRY(launch_mask_dilate(ctx, i_d, rows, cols, r, o_d));
    IMCOM_TRY(st.back(out, (const unsigned char *)o_d, npix));
    return st.done();
}

int imcom_mask_apply(imcom_ctx *ctx, const void *in, int dtype, const unsigned char *mask, long n, void *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(in && mask && out, "null pointer");
    IMCOM_REQUIRE(dtype >= 0 && dtype <= 2, "mask_apply: dtype %d is none of 0 (float32), 1 (float64), 2 (uint8)", dtype);
    IMCOM_REQUIRE(n >= 1 && n <= MASK_MAX_SIDE * MASK_MAX_SIDE, "mask_apply: n = %ld outside 1 .. 2^32", n);
    const size_t esz = dtype == 0 ? 4 : dtype == 1 ? 8 : 1;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, (size_t)n, (size_t)n * esz});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *i_d;
    const unsigned char *m_d;
    char *o_d;
    IMCOM_TRY(st.in((const char *)in, (size_t)n * esz, &i_d));
    IMCOM_TRY(st.in(mask, (size_t)n, &m_d));
    IMCOM_TRY(st.out((char *)out, (size_t)n * esz, &o_d));
    IMCOM_TRY(launch_mask_apply(ctx, i_d, dtype, m_d, n, o_d));
    IMCOM_TRY(st.back((char *)out, (const char *)o_d, (size_t)n * esz));
    return st.done();
}


// ---------------------------------------------------------------------------------------------
// Validation-report statistics: the streaming exact select and the coded-map histogram (quantiles.hip, quantiles_core.h)
}  // extern "C"

struct imcom_quant {
    int S = 0, R = 0, keybits = 32, passes = 3, pass = 0;  // pass: the one being fed; == passes: the results are there
    bool f64 = false, ranks_set = false;
    QtDev d{};
    std::vector<unsigned long long> total0, nan0, hist0;  // what pass 1 counted: elements and NaNs per segment, its histogram [S][QT_BINS]
    std::vector<QtRank> ranks;                            // [S][R]
    std::vector<std::vector<uint64_t>> groups;            // the running pass's live groups per segment
};

namespace {
constexpr int QT_MAX_S = 64, QT_MAX_R = 32;
constexpr long QT_MAX_CHUNK = 1L << 40;
static_assert(QT_BINS == OM_BINS, "a group's counters are one digit's bins");

size_t quant_words(int S, int R) { return (size_t)3 * S + 1 + (size_t)S * R + (size_t)S * R * QT_BINS; }

void quant_digit(const imcom_quant *q, int *shift, int *nbits) { om_digit(q->keybits, q->pass, shift, nbits); }

// zero the running pass's counters and hand the device the groups of q->groups
int quant_arm(imcom_ctx *ctx, imcom_quant *q)
{
    const int S = q->S, R = q->R;
    std::vector<unsigned long long> head((size_t)3 * S + 1 + (size_t)S * R, 0ull);  // tot, nan, ng, bad, gprefix
    for (int s = 0; s < S; s++) {
        head[2 * S + s] = q->groups[s].size();
        for (size_t g = 0; g < q->groups[s].size(); g++) head[3 * S + 1 + (size_t)s * R + g] = q->groups[s][g];
    }
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMCOM_HIP_CHECK(hipMemcpy(q->d.tot, head.data(), head.size() * 8, hipMemcpyHostToDevice));
    for (int s = 0; s < S; s++)
        if (!q->groups[s].empty()) IMCOM_HIP_CHECK(hipMemsetAsync(q->d.hist + (size_t)s * R * QT_BINS, 0, q->groups[s].size() * QT_BINS * 8, ctx->stream));
    return IMCOM_OK;
}

int quant_restart(imcom_ctx *ctx, imcom_quant *q)
{
    q->pass = 0;
    q->ranks_set = false;
    q->groups.assign(q->S, std::vector<uint64_t>(1, 0ull));  // one group a segment holds every key
    return quant_arm(ctx, q);
}

int quant_feedable(const imcom_quant *q, const char *who)
{
    IMCOM_REQUIRE(q, "%s: null accumulator", who);
    IMCOM_REQUIRE(q->pass < q->passes, "%s: every pass has ended (imcom_quant_reset starts over)", who);
    IMCOM_REQUIRE(q->pass == 0 || q->ranks_set, "%s: pass 2 needs the ranks (imcom_quant_set_ranks)", who);
    return IMCOM_OK;
}
}  // namespace

extern "C" {

int imcom_quant_sizes(int n_segments, int n_ranks, int is_f64, long *out)
{
    IMCOM_REQUIRE(out, "null pointer");
    IMCOM_REQUIRE(n_segments >= 1 && n_segments <= QT_MAX_S && n_ranks >= 1 && n_ranks <= QT_MAX_R, "quant: %d segments of %d ranks, served are 1 .. %d of 1 .. %d",
                  n_segments, n_ranks, QT_MAX_S, QT_MAX_R);
    out[0] = (long)(quant_words(n_segments, n_ranks) * 8);
    out[1] = om_passes(is_f64 ? 64 : 32);
    out[2] = QT_BINS;
    out[3] = QT_TILE;
    return IMCOM_OK;
}

int imcom_quant_begin(imcom_ctx *ctx, int n_segments, int n_ranks, int is_f64, void *state, size_t state_bytes, imcom_quant **out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(state && out, "null pointer");
    long sz[4];
    IMCOM_TRY(imcom_quant_sizes(n_segments, n_ranks, is_f64, sz));
    IMCOM_REQUIRE(state_bytes >= (size_t)sz[0] && ((uintptr_t)state & 7) == 0, "quant_begin: state of %zu bytes, needed are %ld (8-byte aligned)", state_bytes, sz[0]);
    imcom_quant *q = new imcom_quant;
    const int S = q->S = n_segments, R = q->R = n_ranks;
    q->f64 = is_f64 != 0;
    q->keybits = q->f64 ? 64 : 32;
    q->passes = om_passes(q->keybits);
    unsigned long long *w = (unsigned long long *)state;
    q->d = QtDev{w, w + S, w + 2 * S, w + 3 * S, w + 3 * S + 1, w + 3 * S + 1 + (size_t)S * R, S, R};
    q->ranks.assign((size_t)S * R, QtRank());
    q->hist0.assign((size_t)S * QT_BINS, 0ull);
    const int rc = quant_restart(ctx, q);
    if (rc != IMCOM_OK) {
        delete q;
        return rc;
    }
    *out = q;
    return IMCOM_OK;
}

int imcom_quant_reset(imcom_ctx *ctx, imcom_quant *q)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(q, "quant_reset: null accumulator");
    return quant_restart(ctx, q);
}

int imcom_quant_free(imcom_ctx *ctx, imcom_quant *q)
{
    IMCOM_TRY(enter(ctx));
    if (q) IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    delete q;
    return IMCOM_OK;
}

int imcom_quant_add_2d(imcom_ctx *ctx, imcom_quant *q, int segment, const void *values, long rows, long cols, long pitch, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(quant_feedable(q, __func__));
    IMCOM_REQUIRE(segment >= 0 && segment < q->S, "quant_add_2d: segment %d of %d", segment, q->S);
    IMCOM_REQUIRE(rows >= 0 && cols >= 0 && pitch >= cols && (rows == 0 || cols == 0 || rows <= QT_MAX_CHUNK / cols), "quant_add_2d: %ld x %ld elements, pitch %ld", rows, cols,
                  pitch);
    if (rows == 0 || cols == 0) return IMCOM_OK;
    IMCOM_REQUIRE(values, "null pointer");
    const size_t esz = q->f64 ? 8 : 4, span = (size_t)(rows - 1) * pitch + cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * esz});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d;
    IMCOM_TRY(st.in((const char *)values, span * esz, &v_d));
    int shift, nbits;
    quant_digit(q, &shift, &nbits);
    IMCOM_TRY(launch_quant_dense(ctx, q->d, q->f64, segment, (int)q->groups[segment].size(), v_d, rows, cols, pitch, shift, nbits));
    return st.done();
}

int imcom_quant_add_flat(imcom_ctx *ctx, imcom_quant *q, const void *values, const void *segment_ids, int ids_i32, long n, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(quant_feedable(q, __func__));
    IMCOM_REQUIRE(n >= 0 && n <= QT_MAX_CHUNK, "quant_add_flat: n = %ld outside 0 .. 2^40", n);
    if (n == 0) return IMCOM_OK;
    IMCOM_REQUIRE(values && segment_ids, "null pointer");
    const size_t esz = q->f64 ? 8 : 4, isz = ids_i32 ? 4 : 1;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {(size_t)n * esz, (size_t)n * isz});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *v_d, *i_d;
    IMCOM_TRY(st.in((const char *)values, (size_t)n * esz, &v_d));
    IMCOM_TRY(st.in((const char *)segment_ids, (size_t)n * isz, &i_d));
    int shift, nbits;
    quant_digit(q, &shift, &nbits);
    IMCOM_TRY(launch_quant_ids(ctx, q->d, q->f64, v_d, i_d, ids_i32 != 0, n, shift, nbits));
    return st.done();
}

int imcom_quant_add_constant(imcom_ctx *ctx, imcom_quant *q, int segment, double value, long count)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(quant_feedable(q, __func__));
    IMCOM_REQUIRE(segment >= 0 && segment < q->S && count >= 0, "quant_add_constant: segment %d of %d, count %ld", segment, q->S, count);
    if (count == 0) return IMCOM_OK;
    int shift, nbits;
    quant_digit(q, &shift, &nbits);
    return launch_quant_constant(ctx, q->d, q->f64, segment, value, (unsigned long long)count, shift, nbits);
}

int imcom_quant_add_rings(imcom_ctx *ctx, imcom_quant *q, const void *frame, int n, long pitch, const double *x, const double *y, int nstar, int rpix, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(quant_feedable(q, __func__));
    IMCOM_REQUIRE(n >= 1 && n <= 32767 && pitch >= n, "quant_add_rings: frame side %d outside 1 .. 32767 (the reference's int16) or pitch %ld below it", n, pitch);
    IMCOM_REQUIRE(rpix >= 1 && rpix <= q->S && rpix <= 4096, "quant_add_rings: %d rings, the accumulator has %d segments", rpix, q->S);
    IMCOM_REQUIRE(nstar >= 0, "quant_add_rings: %d stars", nstar);
    if (nstar == 0) return IMCOM_OK;
    IMCOM_REQUIRE(frame && x && y, "null pointer");
    const size_t esz = q->f64 ? 8 : 4, span = (size_t)(n - 1) * pitch + n;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * esz, (size_t)nstar * 8, (size_t)nstar * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *f_d;
    const double *x_d, *y_d;
    IMCOM_TRY(st.in((const char *)frame, span * esz, &f_d));
    IMCOM_TRY(st.in(x, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(y, (size_t)nstar, &y_d));
    int shift, nbits;
    quant_digit(q, &shift, &nbits);
    IMCOM_TRY(launch_quant_rings(ctx, q->d, q->f64, f_d, n, pitch, x_d, y_d, nstar, rpix, shift, nbits));
    return st.done();
}

int imcom_quant_end_pass(imcom_ctx *ctx, imcom_quant *q, int *passes_left)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_TRY(quant_feedable(q, __func__));
    const int S = q->S, R = q->R;
    std::vector<unsigned long long> head((size_t)3 * S + 1);
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMCOM_HIP_CHECK(hipMemcpy(head.data(), q->d.tot, head.size() * 8, hipMemcpyDeviceToHost));
    const unsigned long long *tot = head.data(), *nan = tot + S, bad = head[3 * S];
    int wrong = -1;
    if (q->pass > 0)
        for (int s = S - 1; s >= 0; s--)
            if (tot[s] != q->total0[s] || nan[s] != q->nan0[s]) wrong = s;
    if (bad || wrong >= 0) {  // the pass did not happen: its counters are zeroed, it can be fed again
        IMCOM_TRY(quant_arm(ctx, q));
        if (bad) set_error("quant_end_pass: %llu segment ids outside 0 .. %d or star positions that are not finite or beyond the int16 range", bad, S - 1);
        else
            set_error("quant_end_pass: pass %d fed segment %d %llu elements (%llu NaN), pass 1 fed it %llu (%llu NaN)", q->pass + 1, wrong, tot[wrong], nan[wrong],
                      q->total0[wrong], q->nan0[wrong]);
        return IMCOM_ERR_ARG;
    }
    std::vector<unsigned long long> hist;
    for (int s = 0; s < S; s++) {
        const size_t ng = q->groups[s].size();
        if (ng == 0) continue;
        hist.resize(ng * QT_BINS);
        IMCOM_HIP_CHECK(hipMemcpy(hist.data(), q->d.hist + (size_t)s * R * QT_BINS, hist.size() * 8, hipMemcpyDeviceToHost));
        if (q->pass == 0) std::copy(hist.begin(), hist.begin() + QT_BINS, q->hist0.begin() + (size_t)s * QT_BINS);
        else qt_advance(q->ranks.data() + (size_t)s * R, R, q->groups[s], (const uint64_t *)hist.data(), q->keybits, q->pass);
    }
    if (q->pass == 0) {
        q->total0.assign(tot, tot + S);
        q->nan0.assign(nan, nan + S);
        for (int s = 0; s < S; s++) q->groups[s].clear();  // until the ranks are set
    }
    q->pass++;
    if (q->pass > 1 && q->pass < q->passes) {
        int shift, nbits;
        quant_digit(q, &shift, &nbits);
        for (int s = 0; s < S; s++) q->groups[s] = qt_groups(q->ranks.data() + (size_t)s * R, R, shift + nbits);
        IMCOM_TRY(quant_arm(ctx, q));
    }
    if (passes_left) *passes_left = q->passes - q->pass;
    return IMCOM_OK;
}

int imcom_quant_counts(imcom_ctx *ctx, const imcom_quant *q, long *total, long *nans)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(q && total && nans, "null pointer");
    IMCOM_REQUIRE(q->pass >= 1, "quant_counts: pass 1 has not ended");
    for (int s = 0; s < q->S; s++) total[s] = (long)q->total0[s], nans[s] = (long)q->nan0[s];
    return IMCOM_OK;
}

int imcom_quant_set_ranks(imcom_ctx *ctx, imcom_quant *q, const long *ranks)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(q && ranks, "null pointer");
    IMCOM_REQUIRE(q->pass == 1, "quant_set_ranks: the ranks are set between pass 1 and pass 2");
    const int S = q->S, R = q->R;
    for (int s = 0; s < S; s++)
        for (int r = 0; r < R; r++) {
            const long k = ranks[(size_t)s * R + r];
            IMCOM_REQUIRE(k >= -1 && (k < 0 || q->total0[s] == 0 || (unsigned long long)k < q->total0[s]), "quant_set_ranks: rank %ld of segment %d with %llu elements", k, s,
                          q->total0[s]);
        }
    const std::vector<uint64_t> all(1, 0ull);
    for (int s = 0; s < S; s++) {
        QtRank *qr = q->ranks.data() + (size_t)s * R;
        const unsigned long long real = q->total0[s] - q->nan0[s];
        for (int r = 0; r < R; r++) {
            const long k = ranks[(size_t)s * R + r];
            qr[r] = QtRank();
            qr[r].live = k >= 0 && (unsigned long long)k < real;
            qr[r].rank = qr[r].live ? (uint64_t)k : 0;
        }
        qt_advance(qr, R, all, (const uint64_t *)q->hist0.data() + (size_t)s * QT_BINS, q->keybits, 0);
    }
    int shift, nbits;
    quant_digit(q, &shift, &nbits);
    for (int s = 0; s < S; s++) q->groups[s] = qt_groups(q->ranks.data() + (size_t)s * R, R, shift + nbits);
    q->ranks_set = true;
    return quant_arm(ctx, q);
}

int imcom_quant_results(imcom_ctx *ctx, const imcom_quant *q, void *out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(q && out, "null pointer");
    IMCOM_REQUIRE(q->pass == q->passes, "quant_results: %d of %d passes have ended", q->pass, q->passes);
    for (size_t i = 0; i < (size_t)q->S * q->R; i++) {
        const QtRank &r = q->ranks[i];
        if (q->f64) ((double *)out)[i] = r.live ? om_value_f64(r.prefix) : std::nan("");
        else ((float *)out)[i] = r.live ? om_value_f32(r.prefix) : std::nanf("");
    }
    return IMCOM_OK;
}

int imcom_codehist(imcom_ctx *ctx, const void *codes, long rows, long cols, long pitch, const unsigned char *table, int nbins, long *counts, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(codes && table && counts, "null pointer");
    IMCOM_REQUIRE(nbins >= 1 && nbins <= 127, "codehist: %d bins outside 1 .. 127", nbins);
    IMCOM_REQUIRE(rows >= 1 && cols >= 1 && pitch >= cols && rows <= QT_MAX_CHUNK / cols, "codehist: %ld x %ld codes, pitch %ld", rows, cols, pitch);
    const size_t span = (size_t)(rows - 1) * pitch + cols;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {span * 2, (size_t)65536, (size_t)(nbins + 1) * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned short *c_d;
    const unsigned char *t_d;
    long *n_d;
    IMCOM_TRY(st.in((const unsigned short *)codes, span, &c_d));
    IMCOM_TRY(st.in(table, (size_t)65536, &t_d));
    IMCOM_TRY(st.out(counts, (size_t)nbins + 1, &n_d));
    IMCOM_TRY(launch_codehist(ctx, c_d, rows, cols, pitch, t_d, nbins, (unsigned long long *)n_d));
    IMCOM_TRY(st.back(counts, (const long *)n_d, (size_t)nbins + 1));
    return st.done();
}

// ---------------------------------------------------------------------------------------------
// The I24 layer codec (i24.hip, i24_core.h)
}  // extern "C"

namespace {
constexpr int I24_MAX_LAYERS = 4096;

// The refusals of the codec and the records the kernels read (rec may be NULL: check only).
int i24_records(int L, long ny, long nx, const imcom_i24_pars *pars, I24Par *rec)
{
    IMCOM_REQUIRE(pars, "i24: null parameters");
    IMCOM_REQUIRE(L >= 1 && L <= I24_MAX_LAYERS, "i24: %d layers, served are 1 .. %d", L, I24_MAX_LAYERS);
    IMCOM_REQUIRE(ny >= 1 && nx >= 1 && ny <= 0x7fffffffL / nx, "i24: %ld x %ld pixels, served are 1 .. 2^31 - 1 a layer", ny, nx);
    for (int l = 0; l < L; l++) {
        const imcom_i24_pars &p = pars[l];
        if (!(p.alpha == 1.0)) {
            set_error("i24: layer %d has ALPHA = %g; only the linear codec (ALPHA absent or 1) is served: the power goes through numpy's float32 pow, whose last bit cannot be reproduced", l, p.alpha);
            return IMCOM_ERR_UNSUPPORTED;
        }
        IMCOM_REQUIRE(std::isfinite(p.vmin) && std::isfinite(p.vmax) && p.vmax > p.vmin, "i24: layer %d has VMIN = %g, VMAX = %g; both must be finite and VMAX > VMIN", l, p.vmin,
                      p.vmax);
        IMCOM_REQUIRE(p.bitkeep >= 1 && p.bitkeep <= 24, "i24: layer %d has BITKEEP = %d outside 1 .. 24", l, p.bitkeep);
        IMCOM_REQUIRE(p.softbias < (1L << 24), "i24: layer %d has SOFTBIAS = %ld; served are 0 .. 2^24 - 1 and -1", l, p.softbias);
        if (!rec) continue;
        I24Par &r = rec[l];
        r.vmin = p.vmin;
        r.range = p.vmax - p.vmin;
        r.vmin_f = (float)p.vmin;
        r.vmax_f = (float)p.vmax;
        r.range_f = (float)r.range;
        r.scale_f = (float)(1 << p.bitkeep);
        r.bitkeep = p.bitkeep;
        r.nb = (p.bitkeep + 7) / 8;
        r.softbias = p.softbias > 0 ? (int)p.softbias : (p.softbias == -1 ? -1 : 0);  // (any other negative value does nothing, as in the reference)
        r.diff = p.diff != 0;
        r.reorder = p.reorder != 0;
        r.pad = 0;
    }
    return IMCOM_OK;
}

long i24_layer_bytes(int L, long n, const imcom_i24_pars *pars, int scheme)
{
    int nb = 1;
    for (int l = 0; l < L; l++) nb = std::max(nb, (pars[l].bitkeep + 7) / 8);
    return scheme == I24_SCHEME_A ? 4 * n : (long)nb * n;
}

size_t i24_state_bytes(int L, long n) { return ((size_t)L * i24_tiles(n) + L) * 4; }

int i24_scheme(int scheme)
{
    IMCOM_REQUIRE(scheme == I24_SCHEME_A || scheme == I24_SCHEME_B, "i24: scheme %d is neither 0 (I24A) nor 1 (I24B)", scheme);
    return IMCOM_OK;
}

int i24_view(long layer_stride, long row_stride, int nx)
{
    IMCOM_REQUIRE(row_stride >= nx && layer_stride >= 0, "i24: a view of rows %ld and layers %ld elements apart for %d columns", row_stride, layer_stride, nx);
    return IMCOM_OK;
}

// layer_off [L + 1] on the device from the host counts; *max_count, *total.
int i24_offsets(imcom_ctx *ctx, int L, const long *counts, long *off_d, long *max_count, long *total)
{
    std::vector<long> off(L + 1, 0);
    *max_count = 0;
    for (int l = 0; l < L; l++) {
        const long c = counts ? counts[l] : 0;
        IMCOM_REQUIRE(c >= 0, "i24: %ld overflow entries for layer %d", c, l);
        off[l + 1] = off[l] + c;
        *max_count = std::max(*max_count, c);
    }
    *total = off[L];
    return upload(ctx, off_d, off.data(), (size_t)L + 1);
}
}  // namespace

extern "C" {

int imcom_i24_sizes(int L, long ny, long nx, const imcom_i24_pars *pars, int scheme, long *out)
{
    IMCOM_REQUIRE(out, "null pointer");
    IMCOM_TRY(i24_scheme(scheme));
    IMCOM_TRY(i24_records(L, ny, nx, pars, nullptr));
    const long n = ny * nx, tiles = i24_tiles(n);
    WsPlan c, d;
    c.add((size_t)L * sizeof(I24Par));
    c.add((size_t)L * n * 4);
    d.add((size_t)L * sizeof(I24Par));
    d.add((size_t)L * n * 4);
    d.add((size_t)L * tiles * 4);
    d.add((size_t)L * 4);
    d.add((size_t)(L + 1) * 8);
    d.add(4);
    out[0] = (long)i24_state_bytes(L, n);
    out[1] = (long)c.total;
    out[2] = (long)d.total;
    out[3] = i24_layer_bytes(L, n, pars, scheme);
    out[4] = tiles;
    out[5] = I24_TILE;
    out[6] = I24_SCAN_CHUNK;
    out[7] = 0;
    return IMCOM_OK;
}

int imcom_i24_compress(imcom_ctx *ctx, const float *frames, long layer_stride, long row_stride, int L, int ny, int nx, const imcom_i24_pars *pars, int scheme,
                       void *out, long out_stride, void *state, size_t state_bytes, long *counts)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(frames && out && state && counts, "null pointer");
    IMCOM_TRY(i24_scheme(scheme));
    std::vector<I24Par> rec((size_t)std::max(L, 1));
    IMCOM_TRY(i24_records(L, ny, nx, pars, rec.data()));
    IMCOM_TRY(i24_view(layer_stride, row_stride, nx));
    const long n = (long)ny * nx, tiles = i24_tiles(n);
    IMCOM_REQUIRE(out_stride >= i24_layer_bytes(L, n, pars, scheme) && (scheme == I24_SCHEME_B || (out_stride % 4 == 0 && ((uintptr_t)out & 3) == 0)),
                  "i24_compress: layers %ld bytes apart in the output, needed are %ld (I24A: int32-aligned)", out_stride, i24_layer_bytes(L, n, pars, scheme));
    IMCOM_REQUIRE(state_bytes >= i24_state_bytes(L, n) && ((uintptr_t)state & 3) == 0, "i24_compress: state of %zu bytes, needed are %zu (4-byte aligned)", state_bytes,
                  i24_state_bytes(L, n));
    WsPlan plan;
    plan.add((size_t)L * sizeof(I24Par));
    plan.add((size_t)L * n * 4);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    I24Par *par_d;
    int *codes;
    IMCOM_TRY(ws_take(ctx, (size_t)L, &par_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L * n, &codes, __func__));
    IMCOM_TRY(upload(ctx, par_d, rec.data(), (size_t)L));
    uint32_t *bases = (uint32_t *)state, *totals = bases + (size_t)L * tiles;
    IMCOM_TRY(launch_i24_quantise(ctx, frames, layer_stride, row_stride, L, ny, nx, par_d, codes, bases, totals));
    IMCOM_TRY(launch_i24_pack(ctx, codes, L, n, par_d, scheme, (unsigned char *)out, out_stride));
    std::vector<uint32_t> tot((size_t)L);
    IMCOM_HIP_CHECK(hipMemcpyAsync(tot.data(), totals, (size_t)L * 4, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int l = 0; l < L; l++) counts[l] = (long)tot[l];
    return IMCOM_OK;
}

int imcom_i24_overflow_fetch(imcom_ctx *ctx, const float *frames, long layer_stride, long row_stride, int L, int ny, int nx, const imcom_i24_pars *pars,
                             const void *state, size_t state_bytes, const long *counts, int *y, int *x, float *value, long capacity)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(frames && state && counts, "null pointer");
    std::vector<I24Par> rec((size_t)std::max(L, 1));
    IMCOM_TRY(i24_records(L, ny, nx, pars, rec.data()));
    IMCOM_TRY(i24_view(layer_stride, row_stride, nx));
    const long n = (long)ny * nx, tiles = i24_tiles(n);
    IMCOM_REQUIRE(state_bytes >= i24_state_bytes(L, n) && ((uintptr_t)state & 3) == 0, "i24_overflow_fetch: state of %zu bytes, needed are %zu (4-byte aligned)", state_bytes,
                  i24_state_bytes(L, n));
    WsPlan plan;
    plan.add((size_t)L * sizeof(I24Par));
    plan.add((size_t)(L + 1) * 8);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    I24Par *par_d;
    long *off_d, max_count, total;
    IMCOM_TRY(ws_take(ctx, (size_t)L, &par_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L + 1, &off_d, __func__));
    IMCOM_TRY(i24_offsets(ctx, L, counts, off_d, &max_count, &total));
    IMCOM_REQUIRE(capacity >= total, "i24_overflow_fetch: a table of %ld entries, the layers have %ld", capacity, total);
    if (total == 0) return IMCOM_OK;
    IMCOM_REQUIRE(y && x && value, "null pointer");
    IMCOM_TRY(upload(ctx, par_d, rec.data(), (size_t)L));
    const uint32_t *bases = (const uint32_t *)state, *totals = bases + (size_t)L * tiles;
    return launch_i24_overflow(ctx, frames, layer_stride, row_stride, L, ny, nx, par_d, bases, totals, off_d, capacity, y, x, value);
}

int imcom_i24_decompress(imcom_ctx *ctx, const void *in, long in_stride, int planes, int scheme, int L, int ny, int nx, const imcom_i24_pars *pars, const int *y,
                         const int *x, const float *value, const long *counts, float *out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(in && out, "null pointer");
    IMCOM_TRY(i24_scheme(scheme));
    std::vector<I24Par> rec((size_t)std::max(L, 1));
    IMCOM_TRY(i24_records(L, ny, nx, pars, rec.data()));
    const long n = (long)ny * nx, tiles = i24_tiles(n);
    bool any_diff = false;
    for (int l = 0; l < L; l++) {
        any_diff = any_diff || rec[l].diff;
        IMCOM_REQUIRE(scheme == I24_SCHEME_A || planes == rec[l].nb, "i24_decompress: a cube of %d byte planes for layer %d, BITKEEP = %d needs %d", planes, l, rec[l].bitkeep,
                      rec[l].nb);
    }
    const long need = scheme == I24_SCHEME_A ? 4 * n : (long)planes * n;
    IMCOM_REQUIRE(in_stride >= need && (scheme == I24_SCHEME_B || (in_stride % 4 == 0 && ((uintptr_t)in & 3) == 0)),
                  "i24_decompress: layers %ld bytes apart in the input, needed are %ld (I24A: int32-aligned)", in_stride, need);
    WsPlan plan;
    plan.add((size_t)L * sizeof(I24Par));
    plan.add((size_t)L * n * 4);
    plan.add((size_t)L * tiles * 4);
    plan.add((size_t)L * 4);
    plan.add((size_t)(L + 1) * 8);
    plan.add(4);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    I24Par *par_d;
    int *codes;
    uint32_t *sums, *totals;
    long *off_d, max_count = 0, total = 0;
    unsigned int *status;
    IMCOM_TRY(ws_take(ctx, (size_t)L, &par_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L * n, &codes, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L * tiles, &sums, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L, &totals, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)L + 1, &off_d, __func__));
    IMCOM_TRY(ws_take(ctx, (size_t)1, &status, __func__));
    if (counts) IMCOM_TRY(i24_offsets(ctx, L, counts, off_d, &max_count, &total));
    IMCOM_REQUIRE(total == 0 || (y && x && value), "i24_decompress: %ld overflow entries and no table", total);
    IMCOM_TRY(upload(ctx, par_d, rec.data(), (size_t)L));
    IMCOM_TRY(launch_i24_decode(ctx, (const unsigned char *)in, in_stride, scheme, L, n, par_d, any_diff, codes, sums, totals, out));
    if (total == 0) return IMCOM_OK;
    IMCOM_HIP_CHECK(hipMemsetAsync(status, 0, 4, ctx->stream));
    IMCOM_TRY(launch_i24_patch(ctx, out, L, ny, nx, off_d, max_count, y, x, value, status));
    unsigned int bad = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(&bad, status, 4, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    IMCOM_REQUIRE(bad == 0, "i24_decompress: the overflow table has a position outside the %d x %d image (it was not stored)", ny, nx);
    return IMCOM_OK;
}

}  // extern "C"
