// i24.hip -- the I24 layer codec of pyimcom.compress (reference src/pyimcom/compress/i24.py, I24Cube.to_mode 367-437 with ALPHA = 1, and
// its helpers lsbf_fwd / lsbf_rev 74-80 / 118-122, diff_fwd / diff_rev 150-154 / 179-181, smallnum_fwd / smallnum_rev 212 / 237) for a batch of
// layers with a parameter record each.  The per-pixel arithmetic, the bit-stream index maps and the dealing of a tile to its threads are
// i24_core.h's; the C-ABI entries imcom_i24_* end the file.
//
// A tile is I24_TILE consecutive flat pixels of one layer; grid = (tiles, layers), one workgroup a tile.  Every output element has one
// owner thread: there is no atomic on data, no read-modify-write of a shared byte, and no kernel waits for another workgroup -- what one
// tile needs from the others (the number of overflow hits before it, the sum of the codes before it) comes from a launch that has ended.
//   compress:   quantise + count  ->  scan of the tile counts  ->  transform + pack       (the table: overflow write, once the caller has room)
//   decompress: unpack (+ tile sums)  ->  scan of the tile sums  ->  prefix sum + dequantise  ->  overflow patch
#include <algorithm>

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

// A batch of L layers of ny x nx pixels (n = ny nx, tiles = i24_tiles(n) of I24_TILE pixels), pars [L] device records.
// launch_i24_quantise: codes [L][n], counts [L][tiles] -> the exclusive prefix sums of the tiles' overflow hits, totals [L].
// launch_i24_pack: codes -> I24A int32 / I24B bytes, layer l at out + l out_stride (bytes).  launch_i24_overflow: the table entries of
// layer l at layer_off[l] .. layer_off[l + 1] (device, [L + 1]) of oy / ox / ov, none at or beyond cap.  launch_i24_decode: in -> codes
// (SOFTBIAS undone), sums [L][tiles] and totals [L] scratch of the prefix sum, out [L][n] float32.  launch_i24_patch: the overflow
// entries into out; *status becomes non-zero if a position lies outside the image (it is not stored).
static int launch_i24_quantise(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, int *codes, uint32_t *counts,
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

static int launch_i24_pack(imcom_ctx *ctx, const int *codes, int L, long n, const I24Par *pars, int scheme, unsigned char *out, long out_stride)
{
    ProfScope ps(ctx, "i24_compress");
    hipLaunchKernelGGL(i24_pack_kernel, dim3((unsigned)i24_tiles(n), (unsigned)L), dim3(I24_THREADS), 0, ctx->stream, codes, n, pars, scheme, out, out_stride);
    return check_launch("i24_pack_kernel");
}

static int launch_i24_overflow(imcom_ctx *ctx, const float *frames, long lstride, long rstride, int L, int ny, int nx, const I24Par *pars, const uint32_t *bases,
                        const uint32_t *totals, const long *layer_off, long cap, int *oy, int *ox, float *ov)
{
    ProfScope ps(ctx, "i24_compress");
    const long n = (long)ny * nx, ntiles = i24_tiles(n);
    hipLaunchKernelGGL(i24_overflow_kernel, dim3((unsigned)ntiles, (unsigned)L), dim3(I24_THREADS), 0, ctx->stream, frames, lstride, rstride, nx, n, ntiles, pars, bases,
                       totals, layer_off, cap, oy, ox, ov);
    return check_launch("i24_overflow_kernel");
}

static int launch_i24_decode(imcom_ctx *ctx, const unsigned char *in, long in_stride, int scheme, int L, long n, const I24Par *pars, bool any_diff, int *codes, uint32_t *sums,
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

static int launch_i24_patch(imcom_ctx *ctx, float *out, int L, int ny, int nx, const long *layer_off, long max_count, const int *oy, const int *ox, const float *ov,
                     unsigned int *status)
{
    ProfScope ps(ctx, "i24_decompress");
    const long gx = std::max(1L, std::min((max_count + 255) / 256, 4L * ctx->cu_count));
    hipLaunchKernelGGL(i24_patch_kernel, dim3((unsigned)gx, (unsigned)L), dim3(256), 0, ctx->stream, out, ny, nx, (long)ny * nx, layer_off, oy, ox, ov, status);
    return check_launch("i24_patch_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: The I24 layer codec (i24_core.h)

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
