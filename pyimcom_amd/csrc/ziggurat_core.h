// ziggurat_core.h -- numpy's float64 normal draw (random_standard_normal of numpy/random/src/distributions/distributions.c) restated by
// stream position, without a device in it.  Compiles as host code too (tests/native/ziggurat_check.cpp).
//
// numpy draws a normal by attempts.  An attempt takes one 64-bit output w of the bit generator: idx = w & 0xff, sign = (w >> 8) & 1,
// rabs = (w >> 9) & (2^52 - 1), x = rabs wi[idx] (negated if sign).  rabs < ki[idx] returns x (99.3 % of attempts).  Otherwise, idx != 0
// (a wedge) takes one more output u and returns x if (fi[idx-1] - fi[idx]) u + fi[idx] < exp(-x^2 / 2), else the draw starts over with a
// new attempt; idx = 0 (the tail) takes pairs of outputs (u1, u2) until 2 (-log1p(-u2)) > (log1p(-u1) / r)^2 and returns
// +-(r - log1p(-u1) / r), the sign from bit 8 of rabs.  So every stream position k has a well-defined "attempt starting at k": it consumes
// a(k) >= 1 outputs and emits a value or not, and the draws are the emitting attempts on the chain k -> k + a(k) from the start.
//
// Two comparisons depend on exp / log1p, whose last bit differs between libms.  Both are evaluated with a relative guard band; a
// comparison inside the band makes the attempt ZIG_UNDECIDED and the caller has the whole request drawn by numpy.  The band: the two
// sides of a comparison are formed from at most four roundings (2^-53 each) and one exp or two log1p; exp's argument x^2 / 2 <= r^2 / 2
// = 6.7 carries a relative rounding of 2^-53, i.e. 6.7 2^-53 in the result; HIP documents exp and log1p of double within 1 ulp, glibc
// within 1 ulp.  Two evaluations of one side therefore differ by less than 16 2^-53 = 2^-49 relative; ZIG_GUARD = 2^-46 is 8 times that.
// How often a call is undecided, from the tables: the left side of a wedge comparison is uniform over [fi[idx], fi[idx-1]], an interval
// of about 1.5 % of its value, so the band of 2 ZIG_GUARD rhs catches 2 ZIG_GUARD fi[idx-1] / (fi[idx-1] - fi[idx]) of the attempts of
// wedge idx: 1.9e-12 of the wedge attempts on average (1.47 % of all attempts are a wedge's), 2.8e-14 per attempt, 4.8e-7 per 4088^2
// draws.  A tail loop longer than ZIG_TAIL_PAIRS pairs is undecided too: a pair is refused with probability E[1 - exp(-E^2 / 2 r^2)] =
// 0.0623 (E exponential), eight in a row 2.3e-10 per tail draw, 2.56e-4 of the attempts are tail draws: 9.8e-7 per 4088^2 draws.
// Together about one white-noise frame in 7 10^5 and one 1/f frame (2^26 draws) in 1.7 10^5 is drawn by numpy on the host.
//
// A tail value itself is a function of log1p's last bit: the device reports where it goes and the two words it is made of, and the
// caller forms it with the libm numpy calls.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ZG_HD __host__ __device__ __forceinline__
#else
#define ZG_HD inline
#endif

namespace imcom {

constexpr int ZIG_TAIL_PAIRS = 8;                // pairs an attempt may take in the tail before it is undecided
constexpr int ZIG_HALO = 2 * ZIG_TAIL_PAIRS;     // outputs an attempt reads beyond its first: a(k) <= ZIG_HALO + 1
constexpr int ZIG_ENTRIES = ZIG_HALO + 1;        // offsets past a tile's start at which the chain can enter it
constexpr double ZIG_R = 3.6541528853610088, ZIG_INV_R = 0.27366123732975828;
constexpr double ZIG_GUARD = 0x1.0p-46;
enum { ZIG_FAST = 0, ZIG_WEDGE = 1, ZIG_REJECT = 2, ZIG_TAIL = 3, ZIG_UNDECIDED = 4 };

struct ZigAttempt {
    int adv;        // outputs consumed, 1 .. ZIG_HALO + 1
    int kind;       // ZIG_FAST / ZIG_WEDGE / ZIG_TAIL emit `value`; ZIG_REJECT and ZIG_UNDECIDED emit nothing
    double value;   // (ZIG_TAIL: this libm's value; the caller's comes from raw[0] and `word`)
    uint64_t word;  // ZIG_TAIL: the output whose log1p is in the value
};

ZG_HD double zig_uniform(uint64_t w) { return (double)(w >> 11) * 0x1.0p-53; }
ZG_HD bool zig_emits(int kind) { return kind == ZIG_FAST || kind == ZIG_WEDGE || kind == ZIG_TAIL; }

// The attempt whose first output is raw[0]; raw[1 .. ZIG_HALO] are readable.
ZG_HD ZigAttempt zig_attempt(const uint64_t *raw, const double *wi, const uint64_t *ki, const double *fi, double guard)
{
    const uint64_t w = raw[0];
    const int idx = (int)(w & 0xff), sign = (int)((w >> 8) & 1);
    const uint64_t rabs = (w >> 9) & 0x000fffffffffffffull;
    double x = (double)rabs * wi[idx];
    if (sign) x = -x;
    ZigAttempt a = {1, ZIG_FAST, x, 0};
    if (rabs < ki[idx]) return a;
    if (idx == 0) {
        for (int pair = 0; pair < ZIG_TAIL_PAIRS; pair++) {
            const double xx = -ZIG_INV_R * log1p(-zig_uniform(raw[1 + 2 * pair]));
            const double yy = -log1p(-zig_uniform(raw[2 + 2 * pair]));
            const double lhs = yy + yy, rhs = xx * xx;
            if (fabs(lhs - rhs) <= guard * fmax(lhs, rhs)) break;
            if (lhs > rhs) {
                a.adv = 3 + 2 * pair;
                a.kind = ZIG_TAIL;
                a.value = ((rabs >> 8) & 1) ? -(ZIG_R + xx) : ZIG_R + xx;
                a.word = raw[1 + 2 * pair];
                return a;
            }
        }
        a.kind = ZIG_UNDECIDED;
        return a;
    }
    const double lhs = (fi[idx - 1] - fi[idx]) * zig_uniform(raw[1]) + fi[idx], rhs = exp(-0.5 * x * x);
    a.adv = 2;
    if (fabs(lhs - rhs) <= guard * rhs) {
        a.adv = 1;
        a.kind = ZIG_UNDECIDED;
    } else {
        a.kind = lhs < rhs ? ZIG_WEDGE : ZIG_REJECT;
    }
    return a;
}

}  // namespace imcom

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host: the tile scheme of ziggurat.hip, step for step ------------------------------------------------------------------------------
// A tile is P consecutive stream positions.  The chain enters it at offset e <= ZIG_HALO past its start (an attempt of the tile before may
// reach that far) and leaves it at an offset of the same range past its end.  Phase A/B: every position's next = k + a(k) and emit flag,
// then next^(2^i) and emit counts by pointer doubling (positions >= P absorb), which gives exit offset and emit count of every entry.
// Phase C: entry and output base of every tile, tile by tile.  Phase D: the on-chain positions of a tile by doubling from its entry
// (positions at chain index a multiple of 2^l mark those 2^l further, l descending), ranks by a prefix sum, values to base + rank.
#include <vector>

namespace imcom {

struct ZigTileMap {
    unsigned char exit[ZIG_ENTRIES];
    unsigned short count[ZIG_ENTRIES];
};

inline int zig_levels(int P)
{
    int l = 0;
    while ((1 << l) < P) l++;
    return l;
}

// raw: the P + ZIG_HALO outputs from the tile's start
inline ZigTileMap zig_tile_map(const uint64_t *raw, int P, const double *wi, const uint64_t *ki, const double *fi, double guard)
{
    const int n = P + ZIG_ENTRIES;
    std::vector<unsigned short> nxt[2] = {std::vector<unsigned short>(n), std::vector<unsigned short>(n)}, cnt[2] = {nxt[0], nxt[0]};
    for (int p = 0; p < n; p++) {
        nxt[0][p] = (unsigned short)p;
        cnt[0][p] = 0;
        if (p < P) {
            const ZigAttempt a = zig_attempt(raw + p, wi, ki, fi, guard);
            nxt[0][p] = (unsigned short)(p + a.adv);
            cnt[0][p] = zig_emits(a.kind) ? 1 : 0;
        }
    }
    int cur = 0;
    for (int l = 0; l <= zig_levels(P); l++, cur ^= 1)
        for (int p = 0; p < n; p++) {
            const int q = nxt[cur][p];
            nxt[cur ^ 1][p] = nxt[cur][q];
            cnt[cur ^ 1][p] = (unsigned short)(cnt[cur][p] + cnt[cur][q]);
        }
    ZigTileMap m;
    for (int e = 0; e < ZIG_ENTRIES; e++) {
        m.exit[e] = (unsigned char)(nxt[cur][e] - P);
        m.count[e] = cnt[cur][e];
    }
    return m;
}

struct ZigDraws {
    std::vector<double> out;          // the draws; a tail draw holds this libm's value
    std::vector<long> tail_idx;       // where the tail draws are
    std::vector<uint64_t> tail_raw;   // [2] each: the attempt's first output, the output whose log1p is in the value
    uint64_t consumed = 0;            // outputs the `count` draws consume
    long slow = 0;                    // consumed attempts that left the fast path
    bool undecided = false, short_of_outputs = false;
};

// Phase D of one tile whose start is stream position `pos0`
inline void zig_tile_emit(const uint64_t *raw, int P, uint64_t pos0, int entry, long base, long count, const double *wi, const uint64_t *ki, const double *fi,
                          double guard, ZigDraws &d)
{
    const int n = P + ZIG_ENTRIES, levels = zig_levels(P) > 0 ? zig_levels(P) : 1;
    std::vector<std::vector<unsigned short>> lev(levels, std::vector<unsigned short>(n));
    std::vector<unsigned char> mark(P, 0);
    for (int p = 0; p < n; p++) lev[0][p] = (unsigned short)(p < P ? p + zig_attempt(raw + p, wi, ki, fi, guard).adv : p);
    for (int l = 1; l < levels; l++)
        for (int p = 0; p < n; p++) lev[l][p] = lev[l - 1][lev[l - 1][p]];
    if (entry < P) mark[entry] = 1;
    for (int l = levels - 1; l >= 0; l--)
        for (int p = 0; p < P; p++)
            if (mark[p] && lev[l][p] < P) mark[lev[l][p]] = 1;
    long r = base;
    for (int p = 0; p < P; p++) {
        if (!mark[p]) continue;
        const ZigAttempt a = zig_attempt(raw + p, wi, ki, fi, guard);
        if (r >= count) break;
        if (a.kind != ZIG_FAST) d.slow++;
        if (a.kind == ZIG_UNDECIDED) d.undecided = true;
        if (!zig_emits(a.kind)) continue;
        d.out[r] = a.value;
        if (a.kind == ZIG_TAIL) {
            d.tail_idx.push_back(r);
            d.tail_raw.push_back(raw[p]);
            d.tail_raw.push_back(a.word);
        }
        if (r == count - 1) d.consumed = pos0 + (uint64_t)lev[0][p];
        r++;
    }
}

// `count` draws from the outputs raw[0 .. nraw), in tiles of P positions
inline ZigDraws zig_draws(const uint64_t *raw_in, long nraw, long count, int P, const double *wi, const uint64_t *ki, const double *fi, double guard)
{
    ZigDraws d;
    d.out.assign((size_t)count, 0.0);
    const long T = (nraw + P - 1) / P;
    std::vector<uint64_t> raw((size_t)(T * P + ZIG_HALO), 0);
    for (long i = 0; i < nraw; i++) raw[(size_t)i] = raw_in[i];
    std::vector<ZigTileMap> maps((size_t)T);
    for (long t = 0; t < T; t++) maps[(size_t)t] = zig_tile_map(raw.data() + t * P, P, wi, ki, fi, guard);
    std::vector<int> entry((size_t)T);
    std::vector<long> base((size_t)T);
    int e = 0;
    long b = 0;
    for (long t = 0; t < T; t++) {
        entry[(size_t)t] = e;
        base[(size_t)t] = b;
        b += maps[(size_t)t].count[e];
        e = maps[(size_t)t].exit[e];
    }
    for (long t = 0; t < T && base[(size_t)t] < count; t++)
        zig_tile_emit(raw.data() + t * P, P, (uint64_t)(t * P), entry[(size_t)t], base[(size_t)t], count, wi, ki, fi, guard, d);
    d.short_of_outputs = b < count || d.consumed > (uint64_t)nraw;
    return d;
}

}  // namespace imcom
#endif
