// ziggurat.hip -- numpy's float64 normal draws of a PCG64 stream (Generator.standard_normal; reference src/pyimcom/layer.py:1303-1304, the
// white-noise layer, and 899-900, the draws of CplxNoise.noise_1f_frame).  The C-ABI entries imcom_pcg64_normal* end the file.
//
// A normal draw consumes a data-dependent number of outputs (ziggurat_core.h), so draw i has no position of its own; but every stream
// position k has an "attempt starting at k" that consumes a(k) outputs, and the draws are the emitting attempts on the chain k -> k + a(k)
// from the start: a list ranking.  The stream is cut into tiles of P positions:
//   zig_map_kernel    (A, B) a workgroup per tile forms the tile's outputs from the closed form of pcg64_dev.h, every position's next and
//                     emit flag, and by pointer doubling in LDS the exit offset and emit count for each of the ZIG_ENTRIES offsets at
//                     which the chain can enter the tile.
//   zig_chain_kernel  (C) entry offset and output base of every tile: one workgroup; a thread composes the maps of a run of tiles for all
//                     entries, one thread chains the 256 run maps, every thread then walks its run from its entry.
//   zig_emit_kernel   (D) a workgroup per tile forms the outputs again (cheaper than storing them), marks the on-chain positions by
//                     doubling from the entry, ranks the emitting ones by a prefix sum and writes value -> out[base + rank]: one owner per
//                     output, no atomics on values, the same bits for every tile size.
// Only integer counters are summed with atomics.  Tail draws (2.7e-4 of all) are listed with their two words; the order of that list
// is the only thing here that can differ from run to run, and the caller sorts it.
#include <algorithm>

#include "launchers.h"
#include "pcg64_dev.h"
#define ZIG_TABLE __device__ const
#include "ziggurat_tables.h"
#include "ziggurat_core.h"

namespace imcom {

namespace {

typedef unsigned long long u64;

// the outputs of stream positions start + tile P + [0, n) into raw[0 .. n): a thread forms a run, one jump and then steps
__device__ __forceinline__ void tile_outputs(const U128 state, const U128 start, long tile, int P, int n, const U128 *tab, u64 *raw)
{
    const int per = (n + (int)blockDim.x - 1) / (int)blockDim.x, i0 = (int)threadIdx.x * per;
    if (i0 >= n) return;
    const u64 add = (u64)tile * (u64)P + (u64)i0, dlo = start.lo + add;
    U128 s = jump(state, dlo, start.hi + (dlo < add), tab);
    const int m = min(per, n - i0);
    for (int q = 0; q < m; q++) raw[i0 + q] = step_output(s, tab);
}

// LDS of both tile kernels: the jump table, then the tile's outputs
constexpr int ZIG_LDS_HEAD = 2 * PCG64_JUMPS * (int)sizeof(U128);

__global__ __launch_bounds__(256) void zig_map_kernel(U128 state, const u64 *__restrict__ jumps, U128 start, int P, int levels, double guard,
                                                      unsigned char *__restrict__ exit_t, unsigned short *__restrict__ count_t)
{
    extern __shared__ u64 lds[];
    U128 *tab = (U128 *)lds;
    u64 *raw = lds + ZIG_LDS_HEAD / 8;                            // [P + ZIG_HALO]
    const int n = P + ZIG_ENTRIES;
    unsigned short *nxt = (unsigned short *)(raw + P + ZIG_HALO);  // [2][n]
    unsigned short *cnt = nxt + 2 * n;                             // [2][n]
    const long tile = blockIdx.x;
    load_jumps(tab, jumps);
    __syncthreads();
    tile_outputs(state, start, tile, P, P + ZIG_HALO, tab, raw);
    __syncthreads();
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        int to = p, emits = 0;
        if (p < P) {
            const ZigAttempt a = zig_attempt((const uint64_t *)raw + p, ZIG_WI, (const uint64_t *)ZIG_KI, ZIG_FI, guard);
            to = p + a.adv;
            emits = zig_emits(a.kind) ? 1 : 0;
        }
        nxt[p] = (unsigned short)to;
        cnt[p] = (unsigned short)emits;
    }
    __syncthreads();
    int cur = 0;
    for (int l = 0; l <= levels; l++, cur ^= 1) {  // 2^(levels + 1) >= 2 P steps: every position has left the tile
        const unsigned short *ni = nxt + cur * n, *ci = cnt + cur * n;
        unsigned short *no = nxt + (cur ^ 1) * n, *co = cnt + (cur ^ 1) * n;
        for (int p = threadIdx.x; p < n; p += blockDim.x) {
            const int q = ni[p];
            no[p] = ni[q];
            co[p] = (unsigned short)(ci[p] + ci[q]);
        }
        __syncthreads();
    }
    if (threadIdx.x < ZIG_ENTRIES) {
        exit_t[tile * ZIG_ENTRIES + threadIdx.x] = (unsigned char)(nxt[cur * n + threadIdx.x] - P);
        count_t[tile * ZIG_ENTRIES + threadIdx.x] = cnt[cur * n + threadIdx.x];
    }
}

// res[0] = the entry offset of the tile after the last, res[1] = the output base there
__global__ __launch_bounds__(256) void zig_chain_kernel(const unsigned char *__restrict__ exit_t, const unsigned short *__restrict__ count_t, long tiles,
                                                        int entry0, long base0, unsigned char *__restrict__ entry_t, long *__restrict__ base_t,
                                                        long *__restrict__ res)
{
    __shared__ unsigned char run_exit[256][ZIG_ENTRIES];
    __shared__ unsigned int run_count[256][ZIG_ENTRIES];
    __shared__ unsigned char run_entry[256];
    __shared__ long run_base[256];
    const int t = threadIdx.x;
    const long per = (tiles + 255) / 256, t0 = min(tiles, t * per), t1 = min(tiles, t0 + per);
    {
        unsigned char cur[ZIG_ENTRIES];
        unsigned int acc[ZIG_ENTRIES];
#pragma unroll
        for (int e = 0; e < ZIG_ENTRIES; e++) {
            cur[e] = (unsigned char)e;
            acc[e] = 0;
        }
        for (long i = t0; i < t1; i++) {
#pragma unroll
            for (int e = 0; e < ZIG_ENTRIES; e++) {
                const long at = i * ZIG_ENTRIES + cur[e];
                acc[e] += count_t[at];
                cur[e] = exit_t[at];
            }
        }
#pragma unroll
        for (int e = 0; e < ZIG_ENTRIES; e++) {
            run_exit[t][e] = cur[e];
            run_count[t][e] = acc[e];
        }
    }
    __syncthreads();
    if (t == 0) {
        int e = entry0;
        long b = base0;
        for (int j = 0; j < 256; j++) {
            run_entry[j] = (unsigned char)e;
            run_base[j] = b;
            b += run_count[j][e];
            e = run_exit[j][e];
        }
        res[0] = e;
        res[1] = b;
    }
    __syncthreads();
    int e = run_entry[t];
    long b = run_base[t];
    for (long i = t0; i < t1; i++) {
        entry_t[i] = (unsigned char)e;
        base_t[i] = b;
        const long at = i * ZIG_ENTRIES + e;
        b += count_t[at];
        e = exit_t[at];
    }
}

// info (device): [0] outputs the `count` draws consume (written by the owner of the last draw), [1] consumed attempts off the fast path,
// [2] tail draws, [3] 1: a consumed attempt was undecided, 2: more tail draws than tail_cap
__global__ __launch_bounds__(256) void zig_emit_kernel(U128 state, const u64 *__restrict__ jumps, U128 start, u64 start_rel, int P, int levels, double guard,
                                                       const unsigned char *__restrict__ entry_t, const long *__restrict__ base_t, long count,
                                                       double *__restrict__ out, long *__restrict__ tail_idx, u64 *__restrict__ tail_raw, long tail_cap,
                                                       u64 *__restrict__ info)
{
    extern __shared__ u64 lds[];
    const long tile = blockIdx.x;
    const long base = base_t[tile];
    if (base >= count) return;  // (the whole workgroup)
    U128 *tab = (U128 *)lds;
    u64 *raw = lds + ZIG_LDS_HEAD / 8;                            // [P + ZIG_HALO]
    const int n = P + ZIG_ENTRIES;
    unsigned short *lev = (unsigned short *)(raw + P + ZIG_HALO);  // [levels][n]: next^(2^l)
    unsigned int *scan = (unsigned int *)(lev + (size_t)levels * n + ((size_t)levels * n & 1));  // [256]
    unsigned char *kind = (unsigned char *)(scan + 256);           // [P]
    unsigned char *mark = kind + P;                                // [P]
    const int t = threadIdx.x;
    load_jumps(tab, jumps);
    __syncthreads();
    tile_outputs(state, start, tile, P, P + ZIG_HALO, tab, raw);
    __syncthreads();
    for (int p = t; p < n; p += blockDim.x) {
        int to = p;
        if (p < P) {
            const ZigAttempt a = zig_attempt((const uint64_t *)raw + p, ZIG_WI, (const uint64_t *)ZIG_KI, ZIG_FI, guard);
            to = p + a.adv;
            kind[p] = (unsigned char)a.kind;
            mark[p] = 0;
        }
        lev[p] = (unsigned short)to;
    }
    __syncthreads();
    for (int l = 1; l < levels; l++) {
        const unsigned short *li = lev + (size_t)(l - 1) * n;
        unsigned short *lo = lev + (size_t)l * n;
        for (int p = t; p < n; p += blockDim.x) lo[p] = li[li[p]];
        __syncthreads();
    }
    const int entry = entry_t[tile];
    if (t == 0 && entry < P) mark[entry] = 1;
    __syncthreads();
    // level l: the marked positions are those at a chain index that is a multiple of 2^(l + 1); each marks the one 2^l further.  (A
    // position marked in this very pass may act too: what it marks is 2^(l + 1) past a marked one, so marked already.)
    for (int l = levels - 1; l >= 0; l--) {
        const unsigned short *ll = lev + (size_t)l * n;
        for (int p = t; p < P; p += blockDim.x)
            if (mark[p]) {
                const int q = ll[p];
                if (q < P) mark[q] = 1;
            }
        __syncthreads();
    }
    // ranks: a thread owns `per` consecutive positions
    const int per = (P + (int)blockDim.x - 1) / (int)blockDim.x, p0 = min(P, t * per), p1 = min(P, p0 + per);
    unsigned int mine = 0;
    for (int p = p0; p < p1; p++) mine += (mark[p] && zig_emits(kind[p])) ? 1u : 0u;
    scan[t] = mine;
    __syncthreads();
    for (int off = 1; off < (int)blockDim.x; off <<= 1) {
        const unsigned int v = t >= off ? scan[t - off] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    long r = base + (long)(scan[t] - mine);
    unsigned int slow = 0, flags = 0;
    for (int p = p0; p < p1 && r < count; p++) {
        if (!mark[p]) continue;
        const int k = kind[p];
        if (k != ZIG_FAST) slow++;
        if (k == ZIG_UNDECIDED) flags |= 1u;
        if (!zig_emits(k)) continue;
        const ZigAttempt a = zig_attempt((const uint64_t *)raw + p, ZIG_WI, (const uint64_t *)ZIG_KI, ZIG_FI, guard);
        out[r] = a.value;
        if (k == ZIG_TAIL) {
            const long slot = (long)atomicAdd(&info[2], 1ull);
            if (slot < tail_cap) {
                tail_idx[slot] = r;
                tail_raw[2 * slot] = raw[p];
                tail_raw[2 * slot + 1] = a.word;
            } else {
                flags |= 2u;
            }
        }
        if (r == count - 1) info[0] = start_rel + (u64)tile * (u64)P + (u64)lev[p];
        r++;
    }
    if (slow) atomicAdd(&info[1], (u64)slow);
    if (flags) atomicOr(&info[3], (u64)flags);
}

}  // namespace

static size_t zig_lds_bytes(int P, int levels)
{
    const size_t n = (size_t)P + ZIG_ENTRIES, head = ZIG_LDS_HEAD + ((size_t)P + ZIG_HALO) * 8;
    const size_t map = head + 4 * n * 2, emit = head + align_up((size_t)levels * n * 2, 4) + 256 * 4 + 2 * (size_t)P;
    return map > emit ? map : emit;
}

// One chunk of `tiles` tiles of P positions from stream position `start` (128 bits; start_rel: the same counted from the call's offset).
// The chain enters the chunk at offset entry0 with base0 draws made; res[2] = {entry offset after the chunk, draws made by then}.
// exit_t / count_t [tiles][ZIG_ENTRIES], entry_t / base_t [tiles]: the tile tables.  info [4] (device, zeroed by the caller): outputs
// consumed by `count` draws, slow attempts, tail draws, flags (1 undecided, 2 tail list full).
static int launch_zig_chunk(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const unsigned long long start[2],
                     unsigned long long start_rel, int P, long tiles, int entry0, long base0, double guard, unsigned char *exit_t, unsigned short *count_t,
                     unsigned char *entry_t, long *base_t, long *res, long count, double *out, long *tail_idx, unsigned long long *tail_raw, long tail_cap,
                     unsigned long long *info)
{
    int levels = 0;
    while ((1 << levels) < P) levels++;
    const int emit_levels = levels > 0 ? levels : 1;
    const unsigned lds = (unsigned)zig_lds_bytes(P, emit_levels);
    const U128 s{state[0], state[1]}, st{start[0], start[1]};
    {
        ProfScope ps(ctx, "zig_map");
        hipLaunchKernelGGL(zig_map_kernel, dim3((unsigned)tiles), dim3(256), lds, ctx->stream, s, jumps, st, P, levels, guard, exit_t, count_t);
        IMCOM_TRY(check_launch("zig_map_kernel"));
    }
    {
        ProfScope ps(ctx, "zig_chain");
        hipLaunchKernelGGL(zig_chain_kernel, dim3(1), dim3(256), 0, ctx->stream, exit_t, count_t, tiles, entry0, base0, entry_t, base_t, res);
        IMCOM_TRY(check_launch("zig_chain_kernel"));
    }
    ProfScope ps(ctx, "zig_emit");
    hipLaunchKernelGGL(zig_emit_kernel, dim3((unsigned)tiles), dim3(256), lds, ctx->stream, s, jumps, st, start_rel, P, emit_levels, guard, entry_t, base_t,
                       count, out, tail_idx, tail_raw, tail_cap, info);
    return check_launch("zig_emit_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: numpy's normal draws of a PCG64 stream

namespace {
constexpr int ZIG_TILE_DEFAULT = 1024, ZIG_TILE_MAX = 1024;  // (the LDS of zig_emit_kernel: 36 KB at 1024)
constexpr long ZIG_CHUNK_TILES_DEFAULT = 1L << 16, ZIG_CHUNK_TILES_MAX = 1L << 20;
constexpr double ZIG_GUARD_DEFAULT = ZIG_GUARD;
// the tiles one chunk may need for `remaining` draws: 1.0145 outputs a draw on average, 3 % and a tile allowed for
long zig_tiles_for(long remaining, int P) { return (remaining + remaining / 32 + P - 1) / P + 1; }
}  // namespace

extern "C" {

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

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// C entries: numpy's Poisson draws of a PCG64 stream and the nstar layer made of them (the kernels and the launch sequence: poisson.hip)

namespace {
int poisson_entry(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long inc[2], const unsigned long long offset[2], const double *lam,
                  const double *brightness, double tot_int, double bg, long count, long *out_i64, float *out_f32, uint64_t *info, int memspace, int S, int W, int T,
                  double guard, int force_walk, const char *who)
{
    IMCOM_TRY(enter(ctx));
    size_t ws = 0, scratch = 0;
    IMCOM_TRY(pcg64_poisson_plan(count, &S, &W, &T, &guard, &ws, &scratch));
    IMCOM_REQUIRE(info && (count == 0 || ((lam || brightness) && (out_i64 || out_f32))), "null pointer");
    for (int i = 0; i < 4; i++) info[i] = 0;
    if (count == 0) return IMCOM_OK;
    Stage st(ctx, memspace, who);
    WsPlan plan;
    plan.add(ws);
    st.plan(plan, {(size_t)count * 8, (size_t)count * (out_i64 ? 8 : 4)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *l_d = nullptr, *b_d = nullptr;
    long *o_d = nullptr;
    float *f_d = nullptr;
    IMCOM_TRY(st.in(brightness ? brightness : lam, (size_t)count, brightness ? &b_d : &l_d));
    if (out_i64)
        IMCOM_TRY(st.out(out_i64, (size_t)count, &o_d));
    else
        IMCOM_TRY(st.out(out_f32, (size_t)count, &f_d));
    unsigned long long info_h[4];
    IMCOM_TRY(pcg64_poisson_device(ctx, state, inc, offset, l_d, b_d, tot_int, bg, count, o_d, f_d, S, W, T, guard, force_walk, info_h, who));
    for (int i = 0; i < 4; i++) info[i] = info_h[i];
    IMCOM_REQUIRE(!info_h[3], "%s: a rate is negative, NaN or above 9.223372006484771e+18", who);
    if (out_i64)
        IMCOM_TRY(st.back(out_i64, (const long *)o_d, (size_t)count));
    else
        IMCOM_TRY(st.back(out_f32, (const float *)f_d, (size_t)count));
    return st.done();
}
}  // namespace

extern "C" {

int imcom_pcg64_poisson_sizes(long count, long *workspace_bytes, long *scratch_bytes)
{
    IMCOM_REQUIRE(workspace_bytes && scratch_bytes, "null pointer");
    int S = 0, W = 0, T = 0;
    double guard = -1.0;
    size_t ws = 0, scratch = 0;
    IMCOM_TRY(pcg64_poisson_plan(count, &S, &W, &T, &guard, &ws, &scratch));
    *workspace_bytes = (long)ws;
    *scratch_bytes = (long)scratch;
    return IMCOM_OK;
}

int imcom_pcg64_poisson(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                        const double *lam, long count, long *out, uint64_t *info, int memspace)
{
    return imcom_pcg64_poisson_ex(ctx, state_lo, state_hi, inc_lo, inc_hi, offset_lo, offset_hi, lam, count, out, info, memspace, 0, 0, 0, -1.0, 0);
}

int imcom_pcg64_poisson_ex(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                           const double *lam, long count, long *out, uint64_t *info, int memspace, int superchunk, int window, int tile, double guard_band,
                           int force_walk)
{
    const unsigned long long state[2] = {state_lo, state_hi}, inc[2] = {inc_lo, inc_hi}, offset[2] = {offset_lo, offset_hi};
    return poisson_entry(ctx, state, inc, offset, lam, nullptr, 0.0, 0.0, count, out, nullptr, info, memspace, superchunk, window, tile, guard_band, force_walk,
                         __func__);
}

int imcom_nstar_layer(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                      const double *brightness, double tot_int, double bg, long count, float *out, uint64_t *info, int memspace)
{
    const unsigned long long state[2] = {state_lo, state_hi}, inc[2] = {inc_lo, inc_hi}, offset[2] = {offset_lo, offset_hi};
    return poisson_entry(ctx, state, inc, offset, nullptr, brightness, tot_int, bg, count, nullptr, out, info, memspace, 0, 0, 0, -1.0, 0, __func__);
}

}  // extern "C"
