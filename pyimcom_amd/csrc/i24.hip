// i24.hip -- the I24 layer codec of pyimcom.compress (reference src/pyimcom/compress/i24.py, I24Cube.to_mode 367-437 with ALPHA = 1, and
// its helpers lsbf_fwd / lsbf_rev 74-80 / 118-122, diff_fwd / diff_rev 150-154 / 179-181, smallnum_fwd / smallnum_rev 212 / 237) for a batch of
// layers with a parameter record each.  The per-pixel arithmetic, the bit-stream index maps and the dealing of a tile to its threads are
// i24_core.h's; the C-ABI entries imcom_i24_* are in api.hip.
//
// A tile is I24_TILE consecutive flat pixels of one layer; grid = (tiles, layers), one workgroup a tile.  Every output element has one
// owner thread: there is no atomic on data, no read-modify-write of a shared byte, and no kernel waits for another workgroup -- what one
// tile needs from the others (the number of overflow hits before it, the sum of the codes before it) comes from a launch that has ended.
//   compress:   quantise + count  ->  scan of the tile counts  ->  transform + pack       (the table: overflow write, once the caller has room)
//   decompress: unpack (+ tile sums)  ->  scan of the tile sums  ->  prefix sum + dequantise  ->  overflow patch
#include "launchers.h"
#include "i24_core.h"

namespace imcom {

namespace {

__device__ __forceinline__ uint32_t i24_wave_scan(uint32_t v)  // inclusive, over the wave's 64 lanes
{
    const int lane = threadIdx.x & (I24_WAVE - 1);
#pragma unroll
    for (int d = 1; d < I24_WAVE; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, I24_WAVE);
        if (lane >= d) v += u;
    }
    return v;
}

// The exclusive prefix of v over the workgroup's threads and *total, their sum (wrapping).  lds [I24_WAVES]; every thread calls it.
__device__ __forceinline__ uint32_t i24_block_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const int lane = threadIdx.x & (I24_WAVE - 1), w = threadIdx.x / I24_WAVE;
    const uint32_t inc = i24_wave_scan(v);
    __syncthreads();  // (the previous use of lds has been read)
    if (lane == I24_WAVE - 1) lds[w] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < I24_WAVES; k++) {
        const uint32_t s = lds[k];
        if (k < w) off += s;
        tot += s;
    }
    *total = tot;
    return off + inc - v;
}

// Quantise + count: codes[l][p] and the overflow hits of every tile.  The frame is read once, through a view with unit column stride.
__global__ __launch_bounds__(I24_THREADS) void i24_quantise_kernel(const float *__restrict__ frames, long lstride, long rstride, int nx, long n, long ntiles,
                                                                   const I24Par *__restrict__ pars, int *__restrict__ codes, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t lds[I24_WAVES];
    const int l = blockIdx.y, t = threadIdx.x;
    const I24Par par = pars[l];
    const long p0 = (long)blockIdx.x * I24_TILE;
    const float *frame = frames + (long)l * lstride;
    uint32_t hits = 0;
#pragma unroll
    for (int i = 0; i < I24_ITEMS; i++) {
        const long p = i24_rank_pixel(p0, i, t);
        if (p >= n) break;
        const long y = p / nx;
        const float d = frame[y * rstride + (p - y * nx)];
        hits += i24_overflows(d, par) ? 1u : 0u;
        codes[(long)l * n + p] = i24_quantise(d, par);
    }
    uint32_t total;
    i24_block_scan(hits, lds, &total);
    if (t == 0) counts[(long)l * ntiles + blockIdx.x] = total;
}

// The middle launch of both scans: sums [L][ntiles] -> their exclusive prefix sums in place, totals [L].  One workgroup a layer walks the
// tile sums I24_SCAN_CHUNK at a time with a carry.
__global__ __launch_bounds__(I24_THREADS) void i24_scan_sums_kernel(uint32_t *__restrict__ sums, long ntiles, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t lds[I24_WAVES];
    const int t = threadIdx.x;
    const uint32_t total = i24_scan_chunks(sums + (long)blockIdx.x * ntiles, ntiles, [&](uint32_t *chunk, int cnt, uint32_t carry) {
        const uint32_t v = t < cnt ? chunk[t] : 0u;
        uint32_t tot;
        const uint32_t ex = i24_block_scan(v, lds, &tot);
        if (t < cnt) chunk[t] = carry + ex;
        return carry + tot;
    });
    if (t == 0) totals[blockIdx.x] = total;
}

// Overflow write: a tile with hits ranks them (ballot + popcount inside a wave, slot offsets inside the tile) and writes y, x, value at
// layer_off[l] + base[tile] + rank: ascending flat order, one owner an entry.  An entry beyond the layer's share of the table or beyond
// `cap` is not written.
__global__ __launch_bounds__(I24_THREADS) void i24_overflow_kernel(const float *__restrict__ frames, long lstride, long rstride, int nx, long n, long ntiles,
                                                                   const I24Par *__restrict__ pars, const uint32_t *__restrict__ bases, const uint32_t *__restrict__ totals,
                                                                   const long *__restrict__ layer_off, long cap, int *__restrict__ oy, int *__restrict__ ox,
                                                                   float *__restrict__ ov)
{
    __shared__ unsigned slots[I24_SLOTS];
    const int l = blockIdx.y, t = threadIdx.x, lane = t & (I24_WAVE - 1), w = t / I24_WAVE;
    const long tile = blockIdx.x;
    const uint32_t base = bases[(long)l * ntiles + tile];
    const uint32_t next = tile + 1 < ntiles ? bases[(long)l * ntiles + tile + 1] : totals[l];
    if (next == base) return;  // (uniform: most tiles have no hit and read nothing)
    const I24Par par = pars[l];
    const long p0 = tile * I24_TILE;
    const float *frame = frames + (long)l * lstride;
    float d[I24_ITEMS];
    unsigned long long ballots[I24_ITEMS];
#pragma unroll
    for (int i = 0; i < I24_ITEMS; i++) {
        const long p = i24_rank_pixel(p0, i, t);
        bool hit = false;
        d[i] = 0.f;
        if (p < n) {
            const long y = p / nx;
            d[i] = frame[y * rstride + (p - y * nx)];
            hit = i24_overflows(d[i], par);
        }
        ballots[i] = __ballot(hit);
        if (lane == 0) slots[i24_rank_slot(i, w)] = (unsigned)__popcll(ballots[i]);
    }
    __syncthreads();
    if (t == 0) i24_slot_offsets(slots);
    __syncthreads();
    const long lo = layer_off[l], hi = layer_off[l + 1];
#pragma unroll
    for (int i = 0; i < I24_ITEMS; i++) {
        if (!((ballots[i] >> lane) & 1ull)) continue;
        const long p = i24_rank_pixel(p0, i, t);
        const long e = lo + base + slots[i24_rank_slot(i, w)] + i24_popcount_below(ballots[i], lane);
        if (e >= hi || e >= cap) continue;
        const long y = p / nx;
        oy[e] = (int)y;
        ox[e] = (int)(p - y * nx);
        ov[e] = d[i];
    }
}

// Transform + pack: DIFF and SOFTBIAS of the tile's codes (and of the few past its end that its bytes reach) into LDS once, then I24A's
// int32 image, I24B's byte planes, or with REORDER the bytes of the bit streams that this tile owns (i24_tile_bytes), every plane of a
// byte from one gather.
__global__ __launch_bounds__(I24_THREADS) void i24_pack_kernel(const int *__restrict__ codes, long n, const I24Par *__restrict__ pars, int scheme,
                                                               unsigned char *__restrict__ out, long out_stride)
{
    __shared__ int mainc[I24_TILE + I24_HALO];
    __shared__ int wrapc[I24_HALO + 1];
    const int l = blockIdx.y, t = threadIdx.x;
    const I24Par par = pars[l];
    const long p0 = (long)blockIdx.x * I24_TILE, p1 = p0 + I24_TILE < n ? p0 + I24_TILE : n;
    const int *q = codes + (long)l * n;
    auto transformed = [&](long p) {
        int c = q[p];
        if (par.diff && p > 0) c = i24_diff_fwd(c, q[p - 1], par.bitkeep);
        return i24_softbias_fwd(c, par.bitkeep, par.softbias);
    };
    for (int i = t; i < I24_TILE + I24_HALO; i += I24_THREADS)
        if (p0 + i < n) mainc[i] = transformed(p0 + i);
    if (t < I24_HALO && t < n) wrapc[t] = transformed(t);
    __syncthreads();
    unsigned char *o = out + (long)l * out_stride;
    if (scheme == I24_SCHEME_A) {
        for (int i = t; i < p1 - p0; i += I24_THREADS) ((int *)o)[p0 + i] = mainc[i];
        return;
    }
    if (!par.reorder) {
        for (int j = 0; j < par.nb; j++)
            for (int i = t; i < p1 - p0; i += I24_THREADS) o[(long)j * n + p0 + i] = (unsigned char)(mainc[i] >> (8 * j));
        return;
    }
    auto code_at = [&](long p) { return (p >= p0 && p < p0 + I24_TILE + I24_HALO) ? mainc[p - p0] : wrapc[p]; };
    for (int b = 0; b < 8; b++) {
        long k0, k1;
        i24_tile_bytes(n, p0, p1, b, &k0, &k1);
        const long k = k0 + t;  // (k1 - k0 <= I24_THREADS)
        if (k >= k1) continue;
        const uint32_t planes = i24_gather_planes(k, n, code_at);
        for (int j = 0; j < par.nb; j++) o[(long)j * n + k] = (unsigned char)(planes >> (8 * j));
    }
}

// Unpack: one owner a pixel gathers its bits (I24B), undoes SOFTBIAS and writes the int32 code; with DIFF the tile's wrapping sum.
__global__ __launch_bounds__(I24_THREADS) void i24_unpack_kernel(const unsigned char *__restrict__ in, long in_stride, int scheme, long n, long ntiles,
                                                                 const I24Par *__restrict__ pars, int *__restrict__ codes, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t lds[I24_WAVES];
    const int l = blockIdx.y, t = threadIdx.x;
    const I24Par par = pars[l];
    const long p0 = (long)blockIdx.x * I24_TILE;
    const unsigned char *src = in + (long)l * in_stride;
    uint32_t sum = 0;
#pragma unroll 2
    for (int i = 0; i < I24_ITEMS; i++) {
        const long p = i24_rank_pixel(p0, i, t);
        if (p >= n) break;
        int c = 0;
        if (scheme == I24_SCHEME_A) c = ((const int *)src)[p];
        else
            for (int j = 0; j < par.nb; j++) {
                const unsigned char *plane = src + (long)j * n;
                const unsigned byte = par.reorder ? i24_scatter_byte(p, n, [&](long k) { return plane[k]; }) : plane[p];
                c += (int)(byte << (8 * j));
            }
        c = i24_softbias_rev(c, par.bitkeep, par.softbias);
        codes[(long)l * n + p] = c;
        sum += (uint32_t)c;
    }
    if (!par.diff) return;  // (uniform)
    uint32_t total;
    i24_block_scan(sum, lds, &total);
    if (t == 0) sums[(long)l * ntiles + blockIdx.x] = total;
}

// The third launch of the prefix sum, and the dequantisation: with DIFF the inclusive wrapping sum from the tile's base, masked to
// BITKEEP bits (179-181); then 414-415.
__global__ __launch_bounds__(I24_THREADS) void i24_finish_kernel(const int *__restrict__ codes, long n, long ntiles, const I24Par *__restrict__ pars,
                                                                 const uint32_t *__restrict__ bases, float *__restrict__ out)
{
    __shared__ uint32_t lds[I24_WAVES];
    const int l = blockIdx.y, t = threadIdx.x;
    const I24Par par = pars[l];
    const long p0 = (long)blockIdx.x * I24_TILE;
    const int *q = codes + (long)l * n;
    uint32_t v[I24_ITEMS];
    uint32_t run = 0;
#pragma unroll
    for (int e = 0; e < I24_ITEMS; e++) {
        const long p = i24_scan_pixel(p0, t, e);
        v[e] = p < n ? (uint32_t)q[p] : 0u;
        run += v[e];
    }
    if (par.diff) {  // (uniform)
        uint32_t total;
        uint32_t acc = bases[(long)l * ntiles + blockIdx.x] + i24_block_scan(run, lds, &total);
        const uint32_t mask = (1u << par.bitkeep) - 1u;
#pragma unroll
        for (int e = 0; e < I24_ITEMS; e++) {
            acc += v[e];
            v[e] = acc & mask;
        }
    }
#pragma unroll
    for (int e = 0; e < I24_ITEMS; e++) {
        const long p = i24_scan_pixel(p0, t, e);
        if (p < n) out[(long)l * n + p] = i24_dequantise((int)v[e], par);
    }
}

// Overflow patch (417-419): out[y, x] = value.  A position outside the image is never stored: it sets *status.
__global__ __launch_bounds__(256) void i24_patch_kernel(float *__restrict__ out, int ny, int nx, long n, const long *__restrict__ layer_off, const int *__restrict__ oy,
                                                        const int *__restrict__ ox, const float *__restrict__ ov, unsigned int *__restrict__ status)
{
    const int l = blockIdx.y;
    const long lo = layer_off[l], hi = layer_off[l + 1];
    for (long e = lo + (long)blockIdx.x * 256 + threadIdx.x; e < hi; e += (long)gridDim.x * 256) {
        const int y = oy[e], x = ox[e];
        if (y < 0 || y >= ny || x < 0 || x >= nx) {
            atomicOr(status, 1u);
            continue;
        }
        out[(long)l * n + (long)y * nx + x] = ov[e];
    }
}

}  // namespace

int launch_i24_quantise(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, int *codes, uint32_t *counts,
                        uint32_t *totals)
{
    ProfScope ps(ctx, "i24_compress");
    const long n = (long)ny * nx, ntiles = i24_tiles(n);
    hipLaunchKernelGGL(i24_quantise_kernel, dim3((unsigned)ntiles, (unsigned)L), dim3(I24_THREADS), 0, ctx->stream, frames, lstride, rstride, nx, n, ntiles, pars, codes,
                       counts);
    IMCOM_TRY(check_launch("i24_quantise_kernel"));
    hipLaunchKernelGGL(i24_scan_sums_kernel, dim3((unsigned)L), dim3(I24_THREADS), 0, ctx->stream, counts, ntiles, totals);
    return check_launch("i24_scan_sums_kernel");
}

int launch_i24_pack(imcom_ctx *ctx, const int *codes, int L, long n, const I24Par *pars, int scheme, unsigned char *out, long out_stride)
{
    ProfScope ps(ctx, "i24_compress");
    hipLaunchKernelGGL(i24_pack_kernel, dim3((unsigned)i24_tiles(n), (unsigned)L), dim3(I24_THREADS), 0, ctx->stream, codes, n, pars, scheme, out, out_stride);
    return check_launch("i24_pack_kernel");
}

int launch_i24_overflow(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, const uint32_t *bases,
                        const uint32_t *totals, const long *layer_off, long cap, int *oy, int *ox, float *ov)
{
    ProfScope ps(ctx, "i24_compress");
    const long n = (long)ny * nx, ntiles = i24_tiles(n);
    hipLaunchKernelGGL(i24_overflow_kernel, dim3((unsigned)ntiles, (unsigned)L), dim3(I24_THREADS), 0, ctx->stream, frames, lstride, rstride, nx, n, ntiles, pars, bases,
                       totals, layer_off, cap, oy, ox, ov);
    return check_launch("i24_overflow_kernel");
}

int launch_i24_decode(imcom_ctx *ctx, const unsigned char *in, long in_stride, int scheme, int L, long n, const I24Par *pars, bool any_diff, int *codes, uint32_t *sums,
                      uint32_t *totals, float *out)
{
    ProfScope ps(ctx, "i24_decompress");
    const long ntiles = i24_tiles(n);
    const dim3 grid((unsigned)ntiles, (unsigned)L);
    hipLaunchKernelGGL(i24_unpack_kernel, grid, dim3(I24_THREADS), 0, ctx->stream, in, in_stride, scheme, n, ntiles, pars, codes, sums);
    IMCOM_TRY(check_launch("i24_unpack_kernel"));
    if (any_diff) {  // (a layer without DIFF wrote no sums: what the scan makes of its row is not read)
        hipLaunchKernelGGL(i24_scan_sums_kernel, dim3((unsigned)L), dim3(I24_THREADS), 0, ctx->stream, sums, ntiles, totals);
        IMCOM_TRY(check_launch("i24_scan_sums_kernel"));
    }
    hipLaunchKernelGGL(i24_finish_kernel, grid, dim3(I24_THREADS), 0, ctx->stream, codes, n, ntiles, pars, sums, out);
    return check_launch("i24_finish_kernel");
}

int launch_i24_patch(imcom_ctx *ctx, float *out, int L, int ny, int nx, const long *layer_off, long max_count, const int *oy, const int *ox, const float *ov,
                     unsigned int *status)
{
    ProfScope ps(ctx, "i24_decompress");
    const long gx = std::max(1L, std::min((max_count + 255) / 256, 4L * ctx->cu_count));
    hipLaunchKernelGGL(i24_patch_kernel, dim3((unsigned)gx, (unsigned)L), dim3(256), 0, ctx->stream, out, ny, nx, (long)ny * nx, layer_off, oy, ox, ov, status);
    return check_launch("i24_patch_kernel");
}

}  // namespace imcom
