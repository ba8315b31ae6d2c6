// quantiles.hip -- the counting kernels of the validation report's statistics (reference src/pyimcom/diagnostics/layer_diagnostics.py:24-64
// and 102-177, _percentiles_and_delete and the gathering loop of LayerReport.build; src/pyimcom/diagnostics/dynrange.py:140-163 and
// 211-238, the two histograms and the ring profiles of gen_dynrange_data): an exact radix select over data that arrives in chunks, for
// many segments and many ranks at once, and the histogram of a (u)int16-coded map through a table of its 65 536 codes.  The C-ABI entries
// imcom_quant_* / imcom_codehist end the file; the host's walk down the digits is theirs and quantiles_core.h's.
//
// A pass counts, per live group (a segment and a key prefix that one of its ranks has reached) and per value of the pass's digit, the
// elements of the segment whose higher bits equal the prefix.  Every number is an integer added with atomics: one right value, whatever
// the cut into chunks, launches, workgroups and the order of arrival.
//   dense chunks (a strided 2-D view into one segment): 32-bit counters in LDS, QT_TILE groups a launch (64 KiB), merged into the 64-bit
//     global counters with one add per non-empty bin; a pass with more live groups reads the chunk once per tile of groups.
//   chunks with a segment id per element and star rings: sparse, many segments -- 64-bit global atomics, a thread adding a run of equal
//     (group, digit) at once.
#include "launchers.h"
#include "quantiles_core.h"

namespace imcom {

// QtDev: the accumulator's device state (all 64-bit words) -- per segment the elements and the NaNs the running pass has seen and the
// number of its live groups, `bad` one word (segment ids out of range, star positions not served), the ascending prefixes of segment s's
// groups at gprefix[s R ..], the group's counters at hist[(s R + g) QT_BINS ..].
constexpr int QT_BINS = 2048, QT_TILE = 8, QT_THREADS = 512;  // counters of a group; groups whose counters share a workgroup's LDS; its threads
struct QtDev {
    unsigned long long *tot, *nan, *ng, *bad, *gprefix, *hist;
    int S, R;
};

typedef unsigned long long u64;

template <typename T, int TILE>
__global__ __launch_bounds__(QT_THREADS) void qt_dense_kernel(const T *__restrict__ p, long rows, long cols, long pitch, int ngroups, int shift, int nbits, int top,
                                                              const u64 *__restrict__ prefix, u64 *__restrict__ hist, u64 *__restrict__ tot, u64 *__restrict__ nan)
{
    __shared__ unsigned int h[TILE][OM_BINS];
    const int t = threadIdx.x;
    for (int b = t; b < TILE * OM_BINS; b += QT_THREADS) (&h[0][0])[b] = 0;
    __syncthreads();
    u64 pre[TILE];
    for (int g = 0; g < TILE; g++) pre[g] = g < ngroups ? prefix[g] : ~0ull;  // (uniform: scalar registers; ~0 is no prefix: top >= 10)
    const unsigned dmask = (1u << nbits) - 1u;
    unsigned int *last = nullptr;
    unsigned run = 0, nans = 0, seen = 0;
    for (long r = blockIdx.y; r < rows; r += gridDim.y) {
        const T *row = p + r * pitch;
        for (long c = (long)blockIdx.x * QT_THREADS + t; c < cols; c += (long)gridDim.x * QT_THREADS) {
            const T v = row[c];
            seen++;
            if (v != v) {
                nans++;
                continue;
            }
            const u64 key = om_key(v), hi = qt_high(key, top);
            int g = -1;
#pragma unroll
            for (int q = 0; q < TILE; q++)
                if (hi == pre[q]) g = q;
            if (g < 0 || g >= ngroups) continue;
            unsigned int *a = &h[g][(unsigned)(key >> shift) & dmask];
            if (a == last) run++;
            else {
                if (run) atomicAdd(last, run);
                last = a, run = 1;
            }
        }
    }
    if (run) atomicAdd(last, run);
    __syncthreads();
    for (int b = t; b < ngroups * OM_BINS; b += QT_THREADS) {
        const unsigned v = (&h[0][0])[b];
        if (v) atomicAdd(&hist[b], (u64)v);
    }
    if (tot) {  // (the first tile of groups counts the chunk)
        if (seen) atomicAdd(tot, (u64)seen);
        if (nans) atomicAdd(nan, (u64)nans);
    }
}

// What the sparse kernels share: element v of segment s goes to the segment's totals and to the group its prefix belongs to, if any.
struct QtRun {
    u64 *addr = nullptr;
    u64 n = 0;
    __device__ __forceinline__ void add(u64 *a)
    {
        if (a == addr) n++;
        else {
            if (n) atomicAdd(addr, n);
            addr = a, n = 1;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n) atomicAdd(addr, n);
        n = 0, addr = nullptr;
    }
};

template <typename T>
__device__ __forceinline__ void qt_emit(const QtDev &d, int s, T v, int shift, int nbits, int top, QtRun &rt, QtRun &rh)
{
    if (v != v) {
        atomicAdd(&d.nan[s], 1ull);  // (rare)
        rt.add(&d.tot[s]);
        return;
    }
    rt.add(&d.tot[s]);
    const u64 key = om_key(v);
    const int g = qt_find((const uint64_t *)d.gprefix + (long)s * d.R, (int)d.ng[s], qt_high(key, top));
    if (g >= 0) rh.add(&d.hist[((long)s * d.R + g) * OM_BINS + ((unsigned)(key >> shift) & ((1u << nbits) - 1u))]);
}

template <typename T, typename ID>
__global__ __launch_bounds__(256) void qt_ids_kernel(const T *__restrict__ p, const ID *__restrict__ ids, long n, QtDev d, int shift, int nbits, int top)
{
    QtRun rt, rh;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long s = (long)ids[i];
        if (s < 0 || s >= d.S) {
            bad++;
            continue;
        }
        qt_emit(d, (int)s, p[i], shift, nbits, top, rt, rh);
    }
    rt.flush();
    rh.flush();
    if (bad) atomicAdd(d.bad, (u64)bad);
}

// One workgroup a star (dynrange.py:216-228): the pixels of its clipped box, each into the ring floor(r) < rpix of this star.
template <typename T>
__global__ __launch_bounds__(256) void qt_rings_kernel(const T *__restrict__ frame, int n, long pitch, const double *__restrict__ xs, const double *__restrict__ ys, int nstar,
                                                       int rpix, QtDev d, int shift, int nbits, int top)
{
    QtRun rt, rh;
    for (int k = blockIdx.x; k < nstar; k += gridDim.x) {
        const double x = xs[k], y = ys[k];
        const double lim = 32767.0 - rpix - 2;
        if (!(fabs(x) < lim && fabs(y) < lim)) {  // (a NaN too: the reference's int16 would wrap)
            if (threadIdx.x == 0) atomicAdd(d.bad, 1ull);
            continue;
        }
        int x0, x1, y0, y1;
        qt_ring_box(x, rpix, n, &x0, &x1);
        qt_ring_box(y, rpix, n, &y0, &y1);
        const int w = x1 - x0, npx = w * (y1 - y0);  // (<= (2 rpix + 4)^2)
        for (int i = threadIdx.x; i < npx; i += 256) {
            const int row = y0 + i / w, col = x0 + i % w;
            const int j = qt_ring_index(col, row, x, y);
            if (j < rpix) qt_emit(d, j, frame[(long)row * pitch + col], shift, nbits, top, rt, rh);
        }
    }
    rt.flush();
    rh.flush();
}

template <typename T>
__global__ void qt_const_kernel(T v, u64 count, int s, QtDev d, int shift, int nbits, int top)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    d.tot[s] += count;
    if (v != v) {
        d.nan[s] += count;
        return;
    }
    const u64 key = om_key(v);
    const int g = qt_find((const uint64_t *)d.gprefix + (long)s * d.R, (int)d.ng[s], qt_high(key, top));
    if (g >= 0) d.hist[((long)s * d.R + g) * OM_BINS + ((unsigned)(key >> shift) & ((1u << nbits) - 1u))] += count;
}

// counts[table[code]] += 1 over a strided view of 16-bit codes (the raw bit pattern indexes the table).  A table value t < 128 is bin t;
// t >= 128 other than 255 is bin t - 128 and bin `nbins` (off scale high) too; 255 is no bin.
__global__ __launch_bounds__(256) void codehist_kernel(const unsigned short *__restrict__ codes, long rows, long cols, long pitch, const unsigned char *__restrict__ table,
                                                       int nbins, u64 *__restrict__ counts)
{
    __shared__ unsigned int h[256];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    int last = -1;
    unsigned run = 0;
    for (long r = blockIdx.y; r < rows; r += gridDim.y) {
        const unsigned short *row = codes + r * pitch;
        for (long c = (long)blockIdx.x * 256 + t; c < cols; c += (long)gridDim.x * 256) {
            const int v = table[row[c]];
            if (v == last) run++;
            else {
                if (run) atomicAdd(&h[last], run);
                last = v, run = 1;
            }
        }
    }
    if (run) atomicAdd(&h[last], run);
    __syncthreads();
    const unsigned v = h[t];
    if (v == 0 || t == 255) return;
    const int bin = t & 127;
    if (bin <= nbins) atomicAdd(&counts[bin], (u64)v);
    if (t >= 128 && bin < nbins) atomicAdd(&counts[nbins], (u64)v);
}

// ------------------------------------------------------------------------------------------------
static dim3 qt_grid(imcom_ctx *ctx, long rows, long cols, int threads)
{
    const long cap = 8L * ctx->cu_count;
    const long gx = std::max(1L, std::min((cols + threads - 1) / threads, cap));
    const long gy = std::max(1L, std::min(rows, std::max(1L, cap / gx)));
    return dim3((unsigned)gx, (unsigned)gy);
}

template <typename T>
static int qt_dense_t(imcom_ctx *ctx, const QtDev &d, int seg, int ng, const T *p, long rows, long cols, long pitch, int shift, int nbits)
{
    const int top = shift + nbits;
    const dim3 grid = qt_grid(ctx, rows, cols, QT_THREADS);
    for (int g0 = 0; g0 < std::max(ng, 1); g0 += QT_TILE) {  // (no live group: the chunk is still counted)
        const int gc = std::min(QT_TILE, ng - g0);
        const u64 *pre = d.gprefix + (long)seg * d.R + g0;
        u64 *hist = d.hist + ((long)seg * d.R + g0) * OM_BINS, *tot = g0 == 0 ? d.tot + seg : nullptr, *nan = d.nan + seg;
        if (gc <= 1) hipLaunchKernelGGL((qt_dense_kernel<T, 1>), grid, dim3(QT_THREADS), 0, ctx->stream, p, rows, cols, pitch, gc, shift, nbits, top, pre, hist, tot, nan);
        else hipLaunchKernelGGL((qt_dense_kernel<T, QT_TILE>), grid, dim3(QT_THREADS), 0, ctx->stream, p, rows, cols, pitch, gc, shift, nbits, top, pre, hist, tot, nan);
        IMCOM_TRY(check_launch("qt_dense_kernel"));
    }
    return IMCOM_OK;
}

static int launch_quant_dense(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, int ng, const void *p, long rows, long cols, long pitch, int shift, int nbits)
{
    ProfScope ps(ctx, "quant_dense");
    return f64 ? qt_dense_t(ctx, d, seg, ng, (const double *)p, rows, cols, pitch, shift, nbits) : qt_dense_t(ctx, d, seg, ng, (const float *)p, rows, cols, pitch, shift, nbits);
}

static int launch_quant_ids(imcom_ctx *ctx, const QtDev &d, bool f64, const void *p, const void *ids, bool ids_i32, long n, int shift, int nbits)
{
    ProfScope ps(ctx, "quant_sparse");
    const dim3 grid((unsigned)std::max(1L, std::min((n + 255) / 256, 8L * ctx->cu_count)));
    const int top = shift + nbits;
    if (f64 && ids_i32) hipLaunchKernelGGL((qt_ids_kernel<double, int>), grid, dim3(256), 0, ctx->stream, (const double *)p, (const int *)ids, n, d, shift, nbits, top);
    else if (f64) hipLaunchKernelGGL((qt_ids_kernel<double, unsigned char>), grid, dim3(256), 0, ctx->stream, (const double *)p, (const unsigned char *)ids, n, d, shift, nbits, top);
    else if (ids_i32) hipLaunchKernelGGL((qt_ids_kernel<float, int>), grid, dim3(256), 0, ctx->stream, (const float *)p, (const int *)ids, n, d, shift, nbits, top);
    else hipLaunchKernelGGL((qt_ids_kernel<float, unsigned char>), grid, dim3(256), 0, ctx->stream, (const float *)p, (const unsigned char *)ids, n, d, shift, nbits, top);
    return check_launch("qt_ids_kernel");
}

static int launch_quant_rings(imcom_ctx *ctx, const QtDev &d, bool f64, const void *frame, int n, long pitch, const double *x, const double *y, int nstar, int rpix, int shift,
                       int nbits)
{
    ProfScope ps(ctx, "quant_sparse");
    const dim3 grid((unsigned)std::max(1, std::min(nstar, 16 * ctx->cu_count)));
    const int top = shift + nbits;
    if (f64) hipLaunchKernelGGL(qt_rings_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)frame, n, pitch, x, y, nstar, rpix, d, shift, nbits, top);
    else hipLaunchKernelGGL(qt_rings_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)frame, n, pitch, x, y, nstar, rpix, d, shift, nbits, top);
    return check_launch("qt_rings_kernel");
}

static int launch_quant_constant(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, double value, unsigned long long count, int shift, int nbits)
{
    const int top = shift + nbits;
    if (f64) hipLaunchKernelGGL(qt_const_kernel<double>, dim3(1), dim3(1), 0, ctx->stream, value, count, seg, d, shift, nbits, top);
    else hipLaunchKernelGGL(qt_const_kernel<float>, dim3(1), dim3(1), 0, ctx->stream, (float)value, count, seg, d, shift, nbits, top);
    return check_launch("qt_const_kernel");
}

static int launch_codehist(imcom_ctx *ctx, const unsigned short *codes, long rows, long cols, long pitch, const unsigned char *table, int nbins, unsigned long long *counts)
{
    ProfScope ps(ctx, "codehist");
    IMCOM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(nbins + 1) * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(codehist_kernel, qt_grid(ctx, rows, cols, 256), dim3(256), 0, ctx->stream, codes, rows, cols, pitch, table, nbins, counts);
    return check_launch("codehist_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: Validation-report statistics: the streaming exact select and the coded-map histogram (quantiles_core.h)

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

}  // extern "C"
