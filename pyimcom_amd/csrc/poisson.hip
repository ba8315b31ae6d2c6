// poisson.hip -- numpy's Poisson draws of a PCG64 stream (Generator.poisson(lam = array); reference src/pyimcom/layer.py:1385-1387, the noise
// of the nstar layer) and the layer formula fused into them.  The C-ABI entries imcom_pcg64_poisson* / imcom_nstar_layer are with the
// other PCG64 draw entries at the end of ziggurat.hip; they call pcg64_poisson_device below.
//
// Draw i consumes a number of outputs that depends on the outputs AND on lam_i (poisson_core.h), so the draws are a path p_{i+1} = p_i +
// c(i, p_i) through the nodes (draw, position).  Draws are taken in ascending superchunks of S; a superchunk's entry position is a device
// scalar the superchunk before wrote, and the host queues every launch without waiting:
//   poi_prep_kernel    (once) per tile of T draws the prefix sums, within its superchunk, of the least consumption m and of the expected
//                      gain of excess; the superchunk totals; the invalid-lam flag.
//   poi_outputs_kernel the stream outputs of the superchunk's position range from the closed form of pcg64_dev.h.
//   poi_map_kernel     a workgroup per tile: layer by layer it evaluates the W window nodes (next excess and flags, in LDS) and moves the
//                      W entry slots of the tile one layer on, which leaves the tile's map entry slot -> exit excess.  A PTRS layer is
//                      evaluated one ATTEMPT per slot -- no lane waits for another's retries, and the slow tests of a layer are taken
//                      together by full waves -- and each slot then follows its refused attempts through the layer.  Eight layers are
//                      evaluated at a time, so their latencies overlap.  The excess every node gains is kept as one byte.
//   poi_group_kernel   the maps of 16 consecutive tiles composed, a thread per entry slot.
//   poi_chain_kernel   one thread chains the group maps from the true entry: the superchunk's exit position, the flags of the path --
//                      off-path nodes never count -- or "the path left a window"; a thread per group then chains its tiles, which
//                      gives every tile's entry excess.
//   poi_values_kernel  a workgroup per tile: one thread follows those bytes from the tile's entry, which places its T draws; a thread
//                      per draw then evaluates it and writes out[i] (or the nstar layer value): one owner per output, no atomics
//                      on values.
//   poi_walk_kernel    one workgroup, one draw after another from the superchunk's entry: the recovery when the path left a window (and
//                      every superchunk with force_walk).  It returns at once otherwise.
// The bits are numpy's for every S, W, T and for the walk; only integer flags and counters are combined with atomics.
#include <algorithm>

#include "launchers.h"
#include "pcg64_dev.h"
#include "poisson_core.h"

namespace imcom {

namespace {

typedef unsigned long long u64;

// where the rates come from: lam[i], or for the nstar layer brightness[i] * tot_int + bg clipped at 0 (layer.py:1385-1386)
struct LamSrc {
    const double *lam, *bright;
    double tot, bg;
};
__device__ __forceinline__ double lam_unclipped(const LamSrc &s, long i) { return s.bright ? s.bright[i] * s.tot + s.bg : s.lam[i]; }
__device__ __forceinline__ double lam_of(const LamSrc &s, long i, bool *valid)
{
    double l = lam_unclipped(s, i);
    if (s.bright && l < 0.0) l = 0.0;  // (np.clip keeps a NaN)
    *valid = poi_lam_valid(l);
    return *valid ? l : 0.0;
}

struct PoiOut {
    long *values;   // int64 draws, or
    float *layer;   // the nstar layer ((P - _lam) + lam) - bg, float64 in that order, rounded to float32 (layer.py:1387)
};
__device__ __forceinline__ void put(const PoiOut &o, const LamSrc &s, long i, long value, double lam)
{
    if (o.values) {
        o.values[i] = value;
    } else {
        const double raw = lam_unclipped(s, i);
        o.layer[i] = (float)((((double)value - lam) + raw) - s.bg);
    }
}

// scinfo [nsc][2]: the superchunk's sum of m, its sum of drift
__global__ __launch_bounds__(256) void poi_prep_kernel(LamSrc src, long count, int S, int T, int *__restrict__ tile_mb, long *__restrict__ tile_D,
                                                       long *__restrict__ scinfo, u64 *__restrict__ info)
{
    __shared__ long sm[256], sd[256];
    const long sc = blockIdx.x, s0 = sc * S;
    const int t = threadIdx.x, ns = (int)min((long)S, count - s0), ntile = (ns + T - 1) / T, tps = S / T;
    const int per = (ntile + 255) / 256, k0 = min(ntile, t * per), k1 = min(ntile, k0 + per);
    long m = 0, d = 0;
    bool bad = false;
    for (int k = k0; k < k1; k++)
        for (int j = k * T; j < min(ns, k * T + T); j++) {
            bool ok;
            const double l = lam_of(src, s0 + j, &ok);
            bad |= !ok;
            m += poi_min_adv(l);
            d += poi_drift256(l);
        }
    sm[t] = m;
    sd[t] = d;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const long vm = t >= off ? sm[t - off] : 0, vd = t >= off ? sd[t - off] : 0;
        __syncthreads();
        sm[t] += vm;
        sd[t] += vd;
        __syncthreads();
    }
    long mb = sm[t] - m, D = sd[t] - d;
    for (int k = k0; k < k1; k++) {
        tile_mb[sc * tps + k] = (int)mb;
        tile_D[sc * tps + k] = D;
        for (int j = k * T; j < min(ns, k * T + T); j++) {
            bool ok;
            const double l = lam_of(src, s0 + j, &ok);
            mb += poi_min_adv(l);
            D += poi_drift256(l);
        }
    }
    if (t == 255) {
        scinfo[2 * sc] = sm[255];
        scinfo[2 * sc + 1] = sd[255];
    }
    if (bad) atomicOr(&info[3], 1ull);
}

// outputs the table kernels of a superchunk may read
__device__ __forceinline__ long poi_need(const long *scinfo, long sc, int W) { return scinfo[2 * sc] + poi_window_lo(scinfo[2 * sc + 1], W) + W + POI_HALO; }

constexpr int POI_RUN = 8;
__global__ __launch_bounds__(256) void poi_outputs_kernel(U128 state, const u64 *__restrict__ jumps, U128 start, const u64 *__restrict__ posv, long sc,
                                                          const long *__restrict__ scinfo, int W, long ucap, u64 *__restrict__ ubuf)
{
    __shared__ U128 tab[2 * PCG64_JUMPS];
    load_jumps(tab, jumps);
    __syncthreads();
    const long need = min(ucap, poi_need(scinfo, sc, W)), i0 = ((long)blockIdx.x * 256 + threadIdx.x) * POI_RUN;
    if (i0 >= need) return;
    const u64 add = posv[sc] + (u64)i0, dlo = start.lo + add;
    U128 s = jump(state, dlo, start.hi + (dlo < add), tab);
    const int n = (int)min((long)POI_RUN, need - i0);
    for (int q = 0; q < n; q++) ubuf[i0 + q] = step_output(s, tab);
}

// poi_map_kernel works through its tile in chunks of L layers, whose nodes are all evaluated before the entry slots move through them
// (the evaluations do not depend on each other; layer by layer their latencies would add up).  LDS: cur [W] ints; acc, fin [L][W] bytes;
// list [L W] shorts; the layers' constants.
constexpr int POI_CHUNK_MAX = 8;
struct PoiLayer {
    PoiPtrs c;
    double lam;
    int m, mb, lo, drift;
};
__host__ __device__ inline int poi_map_chunk(int W, int T) { return max(1, min(min(POI_CHUNK_MAX, T), (61440 / W - 4) / 4)); }
__host__ __device__ inline size_t poi_map_lds(int W, int L) { return (size_t)W * (4 + 4 * L) + 16; }

// A byte of fin / btab: the excess the draw at that layer and window slot gains (2 per refused attempt, X for a mult draw; at most 63) and
// its flags << 6; 255: the node leaves the window.  btab [S][W] keeps them for poi_values_kernel.
__global__ __launch_bounds__(1024) void poi_map_kernel(LamSrc src, long count, long sc, int S, int W, int T, int L, double guard,
                                                       const int *__restrict__ tile_mb, const long *__restrict__ tile_D, const u64 *__restrict__ ubuf,
                                                       int *__restrict__ tilemap, unsigned char *__restrict__ btab)
{
    extern __shared__ int poi_lds[];
    __shared__ PoiLayer lay[POI_CHUNK_MAX];
    __shared__ int nslow;
    int *cur = poi_lds;
    unsigned short *list = (unsigned short *)(cur + W);                // [L W]: layer << 13 | slot is too wide for W = 4096: index l W + w
    unsigned char *acc = (unsigned char *)(list + (size_t)L * W);      // PTRS: POI_ACCEPT / POI_REJECT / POI_SLOW | flags << 4 of the slot's attempt
    unsigned char *fin = acc + (size_t)L * W;
    const long s0 = sc * S;
    const int tile = blockIdx.x, ns = (int)min((long)S, count - s0), j0 = tile * T, j1 = min(ns, j0 + T), nt = blockDim.x, t = threadIdx.x;
    int mb = tile_mb[sc * (S / T) + tile];
    long D = tile_D[sc * (S / T) + tile];
    for (int w = t; w < W; w += nt) cur[w] = poi_window_lo(D, W) + w;
    if (t == 0) nslow = 0;
    for (int jc = j0; jc < j1; jc += L) {
        const int nl = min(L, j1 - jc), nn = nl * W;
        if (t < nl) {
            bool ok;
            PoiLayer &y = lay[t];
            y.lam = lam_of(src, s0 + jc + t, &ok);
            y.m = poi_min_adv(y.lam);
            y.drift = poi_drift256(y.lam);
            if (y.m == 2) y.c = poi_ptrs_consts(y.lam);
        }
        __syncthreads();
        if (t == 0)  // (the running sums are thread 0's alone)
            for (int l = 0; l < nl; l++) {
                lay[l].mb = mb;
                lay[l].lo = poi_window_lo(D, W);
                mb += lay[l].m;
                D += lay[l].drift;
            }
        __syncthreads();
        // every node of the chunk: a PTRS slot's one attempt by the quick tests, any other draw whole
        for (int i = t; i < nn; i += nt) {
            const int l = i / W, w = i - l * W;
            const PoiLayer &y = lay[l];
            const uint64_t *u = (const uint64_t *)ubuf + y.mb + y.lo + w;
            if (y.m == 2) {
                double kf;
                const int r = poi_ptrs_quick(y.c, y.lam, u, &kf);
                acc[i] = (unsigned char)r;
                if (r == POI_SLOW) list[atomicAdd(&nslow, 1)] = (unsigned short)i;  // (the order of the list changes no result; nn <= 65536)
            } else {
                const PoiDraw d = poi_draw(y.lam, u, guard);
                fin[i] = (unsigned char)((d.adv - y.m) | (d.flags << 6));
            }
        }
        __syncthreads();
        const int n = nslow;
        for (int k = t; k < n; k += nt) {  // the slow tests, by full waves
            const int i = list[k], l = i / W, w = i - l * W;
            const PoiLayer &y = lay[l];
            double kf;
            int flags = 0;
            const int r = poi_ptrs_slow(y.c, y.lam, (const uint64_t *)ubuf + y.mb + y.lo + w, guard, &kf, &flags);
            acc[i] = (unsigned char)(r | (flags << 4));
        }
        __syncthreads();
        if (t == 0) nslow = 0;
        for (int i = t; i < nn; i += nt) {  // a PTRS slot follows its refused attempts (slot w -> w + 2) to the accepted one
            const int l = i / W, w = i - l * W;
            if (lay[l].m == 2) {
                int v = w, flags = 0, refused = 0, res = 255;
                while (v < W && refused < POI_PTRS_CAP - 1) {
                    const int a = acc[l * W + v];
                    flags |= a >> 4;
                    if ((a & 3) == POI_ACCEPT) {
                        res = (2 * refused) | (flags << 6);
                        break;
                    }
                    v += 2;
                    refused++;
                }
                fin[i] = (unsigned char)res;
            }
            btab[(long)(jc + l) * W + w] = fin[i];
        }
        __syncthreads();
        for (int w = t; w < W; w += nt) {  // the entry slots through the chunk's layers (slot w of cur is this thread's own)
            int c = cur[w];
            for (int l = 0; l < nl && c >= 0; l++) {
                const int x = c & POI_X_MASK, idx = x - lay[l].lo;
                const int f = idx < 0 || idx >= W ? 255 : fin[l * W + idx];
                c = f == 255 ? POI_LEAVE : ((x + (f & 63)) | (c & ~POI_X_MASK) | ((f >> 6) << POI_X_BITS));
            }
            cur[w] = c;
        }
        __syncthreads();
    }
    for (int w = t; w < W; w += nt) tilemap[(long)tile * W + w] = cur[w];
}

// The maps of G consecutive tiles composed: groupmap [ngroup][W], entry slot of the group's first tile -> exit excess of its last
__global__ __launch_bounds__(1024) void poi_group_kernel(long count, long sc, int S, int W, int T, int G, const long *__restrict__ tile_D,
                                                         const int *__restrict__ tilemap, int *__restrict__ groupmap)
{
    const long s0 = sc * S;
    const int ns = (int)min((long)S, count - s0), ntile = (ns + T - 1) / T, t0 = blockIdx.x * G, t1 = min(ntile, t0 + G);
    const long *tD = tile_D + sc * (S / T);
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        int c = poi_window_lo(tD[t0], W) + w;
        for (int t = t0; t < t1 && c >= 0; t++) {
            const int idx = (c & POI_X_MASK) - poi_window_lo(tD[t], W);
            const int v = idx < 0 || idx >= W ? POI_LEAVE : tilemap[(long)t * W + idx];
            c = v < 0 ? POI_LEAVE : ((v & POI_X_MASK) | ((c | v) & ~POI_X_MASK));
        }
        groupmap[(long)blockIdx.x * W + w] = c;
    }
}

// info (device): [0] unused, [1] flags of the path (POI_UNDECIDED | POI_OVERCAP), [2] superchunks recovered by the walk, [3] invalid lam
constexpr int POI_MAX_GROUPS = 1024;
__global__ __launch_bounds__(256) void poi_chain_kernel(long count, long sc, int S, int W, int T, int G, const long *__restrict__ tile_D,
                                                        const long *__restrict__ scinfo, const int *__restrict__ tilemap, const int *__restrict__ groupmap,
                                                        int *__restrict__ entry, u64 *__restrict__ posv, int *__restrict__ recover, u64 *__restrict__ info)
{
    __shared__ int gentry[POI_MAX_GROUPS];
    __shared__ int left;
    const long s0 = sc * S;
    const int ns = (int)min((long)S, count - s0), ntile = (ns + T - 1) / T, ngroup = (ntile + G - 1) / G;
    const long *tD = tile_D + sc * (S / T);
    if (threadIdx.x == 0) {  // the groups from the true entry, excess 0
        int e = 0, flags = 0;
        left = 0;
        for (int g = 0; g < ngroup; g++) {
            const int idx = e - poi_window_lo(tD[g * G], W);
            const int v = idx < 0 || idx >= W ? POI_LEAVE : groupmap[(long)g * W + idx];
            gentry[g] = e;
            if (v < 0) {
                left = 1;
                break;
            }
            e = v & POI_X_MASK;
            flags |= v >> POI_X_BITS;
        }
        recover[sc] = left;
        if (!left) {
            posv[sc + 1] = posv[sc] + (u64)scinfo[2 * sc] + (u64)e;
            if (flags) atomicOr(&info[1], (u64)flags);
        }
    }
    __syncthreads();
    if (left) return;
    for (int g = threadIdx.x; g < ngroup; g += blockDim.x) {  // every group's tiles from the group's entry (none leaves: its map did not)
        int e = gentry[g];
        for (int t = g * G; t < min(ntile, g * G + G); t++) {
            entry[t] = e;
            e = tilemap[(long)t * W + (e - poi_window_lo(tD[t], W))] & POI_X_MASK;
        }
    }
}

// A workgroup per tile: one thread follows the byte table from the tile's entry through its T layers, which places every draw; then a
// thread per draw evaluates it.  LDS: m [T], drift [T], position [T] ints.
__global__ __launch_bounds__(256) void poi_values_kernel(LamSrc src, long count, long sc, int S, int W, int T, double guard, const int *__restrict__ tile_mb,
                                                         const long *__restrict__ tile_D, const u64 *__restrict__ ubuf, const unsigned char *__restrict__ btab,
                                                         const int *__restrict__ entry, const int *__restrict__ recover, PoiOut out)
{
    if (recover[sc]) return;
    extern __shared__ int poi_lds[];
    int *mj = poi_lds, *dj = poi_lds + T, *pj = poi_lds + 2 * T;
    const long s0 = sc * S;
    const int tile = blockIdx.x, ns = (int)min((long)S, count - s0), j0 = tile * T, nj = min(ns, j0 + T) - j0;
    for (int t = threadIdx.x; t < nj; t += blockDim.x) {
        bool ok;
        const double lam = lam_of(src, s0 + j0 + t, &ok);
        mj[t] = poi_min_adv(lam);
        dj[t] = poi_drift256(lam);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int mb = tile_mb[sc * (S / T) + tile], x = entry[tile];
        long D = tile_D[sc * (S / T) + tile];
        for (int t = 0; t < nj; t++) {
            pj[t] = mb + x;
            x += btab[(long)(j0 + t) * W + (x - poi_window_lo(D, W))] & 63;  // (on the path: inside the window, never 255)
            mb += mj[t];
            D += dj[t];
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nj; t += blockDim.x) {
        bool ok;
        const double lam = lam_of(src, s0 + j0 + t, &ok);
        const PoiDraw d = poi_draw(lam, (const uint64_t *)ubuf + pj[t], guard);
        put(out, src, s0 + j0 + t, d.value, lam);
    }
}

constexpr int POI_WALK_BUF = 2048;
__global__ __launch_bounds__(256) void poi_walk_kernel(U128 state, const u64 *__restrict__ jumps, U128 start, LamSrc src, long count, long sc, int S,
                                                       double guard, int force, u64 *__restrict__ posv, const int *__restrict__ recover, PoiOut out,
                                                       u64 *__restrict__ info)
{
    if (!force && !recover[sc]) return;
    __shared__ U128 tab[2 * PCG64_JUMPS];
    __shared__ u64 raw[POI_WALK_BUF + POI_HALO];
    __shared__ u64 s_pos;
    __shared__ long s_i;
    const int t = threadIdx.x;
    load_jumps(tab, jumps);
    u64 pos = posv[sc];
    long i = sc * S;
    const long iend = min(count, i + S);
    int flags = 0;
    __syncthreads();
    while (i < iend) {
        constexpr int n = POI_WALK_BUF + POI_HALO, per = (n + 255) / 256;
        const int q0 = t * per;
        if (q0 < n) {
            const u64 add = pos + (u64)q0, dlo = start.lo + add;
            U128 s = jump(state, dlo, start.hi + (dlo < add), tab);
            for (int q = q0; q < min(n, q0 + per); q++) raw[q] = step_output(s, tab);
        }
        __syncthreads();
        if (t == 0) {
            int q = 0;
            while (i < iend && q <= POI_WALK_BUF) {
                bool ok;
                const double lam = lam_of(src, i, &ok);
                const PoiDraw d = poi_draw(lam, (const uint64_t *)raw + q, guard);
                put(out, src, i, d.value, lam);
                flags |= d.flags;
                q += d.adv;
                i++;
            }
            s_pos = pos + (u64)q;
            s_i = i;
        }
        __syncthreads();
        pos = s_pos;
        i = s_i;
        __syncthreads();
    }
    if (t == 0) {
        posv[sc + 1] = pos;
        if (flags) atomicOr(&info[1], (u64)flags);
        if (!force) atomicAdd(&info[2], 1ull);
    }
}

}  // namespace

// Defaults from measurements on an MI355X (tools/bench_poisson.py): the spread of the excess after S draws at lam = 86 is 0.92 sqrt(S), so
// W = 768 is +-4.6 sigma at S = 8192.
constexpr int POI_S_DEFAULT = 8192, POI_W_DEFAULT = 768, POI_T_DEFAULT = 32;

// The parameters of a call: 0 (guard: negative) stands for the default; refusals; the workspace a call of `count` draws takes with
// every array in device memory, and the part of it that is per-superchunk scratch (outputs, tile maps, entries).
int pcg64_poisson_plan(long count, int *S, int *W, int *T, double *guard, size_t *ws_bytes, size_t *scratch_bytes)
{
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64_poisson: count %ld outside 0 .. 2^36", count);
    if (*S == 0) *S = POI_S_DEFAULT;
    if (*W == 0) *W = POI_W_DEFAULT;
    if (*T == 0) *T = std::min(POI_T_DEFAULT, *S);
    if (*guard < 0.0) *guard = POI_GUARD;
    IMCOM_REQUIRE(*T >= 1 && *T <= 4096 && *S >= *T && *S <= 65536 && *S % *T == 0, "pcg64_poisson: superchunks of %d draws in tiles of %d (S a multiple of T, at most 65536)",
                  *S, *T);
    IMCOM_REQUIRE(*W >= 2 && *W <= 4096, "pcg64_poisson: window %d outside 2 .. 4096", *W);
    IMCOM_REQUIRE(*guard <= 1.0, "pcg64_poisson: guard band %g above 1", *guard);
    const long nsc = (count + *S - 1) / *S, tps = *S / *T;
    WsPlan p, q;
    p.add((size_t)PCG64_JUMPS * 32);
    p.add((size_t)(nsc * tps) * 4);  // tile_mb
    p.add((size_t)(nsc * tps) * 8);  // tile_D
    p.add((size_t)nsc * 16);         // scinfo
    p.add((size_t)(nsc + 1) * 8);    // posv
    p.add((size_t)nsc * 4);          // recover
    p.add(4 * sizeof(u64));          // info
    for (WsPlan *w : {&p, &q}) {
        w->add((size_t)(12L * *S + *W + POI_HALO) * 8);  // ubuf
        w->add((size_t)tps * *W * 4);                    // tilemap
        w->add((size_t)tps * 4);                         // entry
        w->add((size_t)*S * *W);                         // btab
        w->add((size_t)std::min<long>(tps, POI_MAX_GROUPS) * *W * 4);  // groupmap
    }
    *ws_bytes = p.total;
    *scratch_bytes = q.total;
    return IMCOM_OK;
}

// The draws of rates lam[i] (or, brightness != null, of max(brightness[i] tot_int + bg, 0)) from stream position `offset` of the stream
// (state, inc); every pointer is device memory; the workspace (pcg64_poisson_plan) has been reserved by the caller.  values: int64
// draws, or layer: the float32 nstar layer.  info_h [4]: outputs consumed, 1 if a draw of the path was undecided or over a cap,
// superchunks recovered by the walk, 1 if a rate is invalid (nothing useful has been written then).  Waits for the stream.
int pcg64_poisson_device(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long inc[2], const unsigned long long offset[2],
                         const double *lam, const double *brightness, double tot_int, double bg, long count, long *values, float *layer, int S, int W, int T,
                         double guard, int force_walk, unsigned long long *info_h, const char *who)
{
    const long nsc = (count + S - 1) / S, tps = S / T, ucap = 12L * S + W + POI_HALO;
    const u64 *jumps;
    int *tile_mb, *recover, *tilemap, *entry, *groupmap;
    unsigned char *btab;
    long *tile_D, *scinfo;
    u64 *posv, *ubuf, *info;
    IMCOM_TRY(pcg64_jumps(ctx, inc[0], inc[1], &jumps, who));
    IMCOM_TRY(ws_take(ctx, (size_t)(nsc * tps), &tile_mb, who));
    IMCOM_TRY(ws_take(ctx, (size_t)(nsc * tps), &tile_D, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nsc * 2, &scinfo, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nsc + 1, &posv, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nsc, &recover, who));
    IMCOM_TRY(ws_take(ctx, (size_t)4, &info, who));
    IMCOM_TRY(ws_take(ctx, (size_t)ucap, &ubuf, who));
    IMCOM_TRY(ws_take(ctx, (size_t)tps * W, &tilemap, who));
    IMCOM_TRY(ws_take(ctx, (size_t)tps, &entry, who));
    IMCOM_TRY(ws_take(ctx, (size_t)S * W, &btab, who));
    IMCOM_TRY(ws_take(ctx, (size_t)std::min<long>(tps, POI_MAX_GROUPS) * W, &groupmap, who));
    const int G = (int)std::max<long>(std::min<long>(16, tps), (tps + POI_MAX_GROUPS - 1) / POI_MAX_GROUPS);  // tiles of a group of the chain
    IMCOM_HIP_CHECK(hipMemsetAsync(info, 0, 4 * sizeof(u64), ctx->stream));
    IMCOM_HIP_CHECK(hipMemsetAsync(posv, 0, sizeof(u64), ctx->stream));
    const U128 s{state[0], state[1]}, st{offset[0], offset[1]};
    const LamSrc src{lam, brightness, tot_int, bg};
    const PoiOut out{values, layer};
    {
        ProfScope ps(ctx, "poi_prep");
        hipLaunchKernelGGL(poi_prep_kernel, dim3((unsigned)nsc), dim3(256), 0, ctx->stream, src, count, S, T, tile_mb, tile_D, scinfo, info);
        IMCOM_TRY(check_launch("poi_prep_kernel"));
    }
    {  // an invalid rate: nothing is written
        u64 bad = 0;
        IMCOM_HIP_CHECK(hipMemcpyAsync(&bad, info + 3, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (bad) {
            info_h[0] = info_h[1] = info_h[2] = 0;
            info_h[3] = 1;
            return IMCOM_OK;
        }
    }
    const int map_threads = std::min(1024, (W + 63) / 64 * 64), L = poi_map_chunk(W, T);
    for (long sc = 0; sc < nsc; sc++) {
        const int ns = (int)std::min<long>(S, count - sc * S), ntile = (ns + T - 1) / T;
        if (!force_walk) {
            {
                ProfScope ps(ctx, "poi_outputs");
                hipLaunchKernelGGL(poi_outputs_kernel, dim3((unsigned)((ucap + 256 * POI_RUN - 1) / (256 * POI_RUN))), dim3(256), 0, ctx->stream, s, jumps, st,
                                   posv, sc, scinfo, W, ucap, ubuf);
                IMCOM_TRY(check_launch("poi_outputs_kernel"));
            }
            {
                ProfScope ps(ctx, "poi_map");
                hipLaunchKernelGGL(poi_map_kernel, dim3((unsigned)ntile), dim3(map_threads), poi_map_lds(W, L), ctx->stream, src, count, sc, S, W, T, L,
                                   guard, tile_mb, tile_D, ubuf, tilemap, btab);
                IMCOM_TRY(check_launch("poi_map_kernel"));
            }
            {
                ProfScope ps(ctx, "poi_chain");
                hipLaunchKernelGGL(poi_group_kernel, dim3((unsigned)((ntile + G - 1) / G)), dim3(map_threads), 0, ctx->stream, count, sc, S, W, T, G, tile_D, tilemap,
                                   groupmap);
                IMCOM_TRY(check_launch("poi_group_kernel"));
                hipLaunchKernelGGL(poi_chain_kernel, dim3(1), dim3(256), 0, ctx->stream, count, sc, S, W, T, G, tile_D, scinfo, tilemap, groupmap, entry, posv,
                                   recover, info);
                IMCOM_TRY(check_launch("poi_chain_kernel"));
            }
            {
                ProfScope ps(ctx, "poi_values");
                hipLaunchKernelGGL(poi_values_kernel, dim3((unsigned)ntile), dim3(std::min(256, (T + 63) / 64 * 64)), (size_t)3 * T * 4, ctx->stream, src, count, sc,
                                   S, W, T, guard, tile_mb, tile_D, ubuf, btab, entry, recover, out);
                IMCOM_TRY(check_launch("poi_values_kernel"));
            }
        }
        ProfScope ps(ctx, "poi_walk");
        hipLaunchKernelGGL(poi_walk_kernel, dim3(1), dim3(256), 0, ctx->stream, s, jumps, st, src, count, sc, S, guard, force_walk, posv, recover, out, info);
        IMCOM_TRY(check_launch("poi_walk_kernel"));
    }
    u64 got[4], consumed = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(got, info, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipMemcpyAsync(&consumed, posv + nsc, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    info_h[0] = consumed;
    info_h[1] = got[1] != 0;
    info_h[2] = got[2];
    info_h[3] = got[3] != 0;
    return IMCOM_OK;
}

}  // namespace imcom
