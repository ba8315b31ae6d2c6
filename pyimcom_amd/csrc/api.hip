// api.hip -- the context: the error text, workspace, staging and profiling helpers every source file calls (common.h), and the extern "C"
// entries imcom_version, imcom_last_error, imcom_device_count and imcom_ctx_* (all but the two probes, which end gemm_f64.hip).  No kernel and
// no launch.  Every seam's entries (include/imcom_hip.h) end the file that holds its kernels; the Cholesky solve's end chol_solve.hip.
#include <cmath>

#include "common.h"

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

}  // extern "C"
