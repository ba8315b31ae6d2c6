// quantiles.hip -- the counting kernels of the validation report's statistics (reference src/pyimcom/diagnostics/layer_diagnostics.py:24-64
// and 102-177, _percentiles_and_delete and the gathering loop of LayerReport.build; src/pyimcom/diagnostics/dynrange.py:140-163 and
// 211-238, the two histograms and the ring profiles of gen_dynrange_data): an exact radix select over data that arrives in chunks, for
// many segments and many ranks at once, and the histogram of a (u)int16-coded map through a table of its 65 536 codes.  The C-ABI entries
// imcom_quant_* / imcom_codehist and the host's walk down the digits are in api.hip and quantiles_core.h.
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

int launch_quant_dense(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, int ng, const void *p, long rows, long cols, long pitch, int shift, int nbits)
{
    ProfScope ps(ctx, "quant_dense");
    return f64 ? qt_dense_t(ctx, d, seg, ng, (const double *)p, rows, cols, pitch, shift, nbits) : qt_dense_t(ctx, d, seg, ng, (const float *)p, rows, cols, pitch, shift, nbits);
}

int launch_quant_ids(imcom_ctx *ctx, const QtDev &d, bool f64, const void *p, const void *ids, bool ids_i32, long n, int shift, int nbits)
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

int launch_quant_rings(imcom_ctx *ctx, const QtDev &d, bool f64, const void *frame, int n, long pitch, const double *x, const double *y, int nstar, int rpix, int shift,
                       int nbits)
{
    ProfScope ps(ctx, "quant_sparse");
    const dim3 grid((unsigned)std::max(1, std::min(nstar, 16 * ctx->cu_count)));
    const int top = shift + nbits;
    if (f64) hipLaunchKernelGGL(qt_rings_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)frame, n, pitch, x, y, nstar, rpix, d, shift, nbits, top);
    else hipLaunchKernelGGL(qt_rings_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)frame, n, pitch, x, y, nstar, rpix, d, shift, nbits, top);
    return check_launch("qt_rings_kernel");
}

int launch_quant_constant(imcom_ctx *ctx, const QtDev &d, bool f64, int seg, double value, unsigned long long count, int shift, int nbits)
{
    const int top = shift + nbits;
    if (f64) hipLaunchKernelGGL(qt_const_kernel<double>, dim3(1), dim3(1), 0, ctx->stream, value, count, seg, d, shift, nbits, top);
    else hipLaunchKernelGGL(qt_const_kernel<float>, dim3(1), dim3(1), 0, ctx->stream, (float)value, count, seg, d, shift, nbits, top);
    return check_launch("qt_const_kernel");
}

int launch_codehist(imcom_ctx *ctx, const unsigned short *codes, long rows, long cols, long pitch, const unsigned char *table, int nbins, unsigned long long *counts)
{
    ProfScope ps(ctx, "codehist");
    IMCOM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(nbins + 1) * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(codehist_kernel, qt_grid(ctx, rows, cols, 256), dim3(256), 0, ctx->stream, codes, rows, cols, pitch, table, nbins, counts);
    return check_launch("codehist_kernel");
}

}  // namespace imcom
