// i24_core.h -- the arithmetic of i24.hip that has one right answer and no device in it (reference src/pyimcom/compress/i24.py): the
// per-pixel steps of the I24 codec (quantise 376-378, DIFF 150-154, SOFTBIAS 383 / 212 / 409 / 237, dequantise 414-415), the index maps of
// the REORDER bit stream (lsbf_fwd 74-80, lsbf_rev 118-122), and how a tile of pixels is dealt to a workgroup's threads for the ranking
// of the overflow table and for the prefix sum.  Compiles as host code too (tests/native/i24_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define I24_HD __host__ __device__ inline
#else
#define I24_HD inline
#endif

namespace imcom {

// A tile is I24_TILE consecutive flat pixels of one layer and belongs to one workgroup of I24_THREADS threads (I24_WAVES waves of
// I24_WAVE lanes), I24_ITEMS pixels a thread.  The scan of the tile sums takes I24_SCAN_CHUNK of them per step of its one workgroup.
constexpr int I24_THREADS = 256, I24_ITEMS = 8, I24_TILE = I24_THREADS * I24_ITEMS, I24_WAVE = 64, I24_WAVES = I24_THREADS / I24_WAVE;
constexpr int I24_SLOTS = I24_ITEMS * I24_WAVES;  // (item, wave) pairs of a tile: the units of the ranking
constexpr int I24_SCAN_CHUNK = I24_THREADS;
constexpr int I24_HALO = 7;  // pixels past a tile's end that a byte owned by the tile can reach
constexpr int I24_SCHEME_A = 0, I24_SCHEME_B = 1;

// The parameters of one layer as the kernels read them (device memory, one record a layer).
struct I24Par {
    double vmin, range;       // VMIN and VMAX - VMIN in float64 (dequantise)
    float vmin_f, vmax_f;     // f32(VMIN), f32(VMAX) (overflow test, clip)
    float range_f, scale_f;   // f32(VMAX - VMIN), f32(2^BITKEEP)
    int bitkeep, nb, softbias, diff, reorder;  // softbias: 0 none, > 0 the bias, -1 smallnum; nb = (BITKEEP + 7) / 8
    int pad;
};

I24_HD long i24_tiles(long n) { return (n + I24_TILE - 1) / I24_TILE; }

// ---- per-pixel arithmetic ---------------------------------------------------------------------------------------------------------------

// 368: d < f32(VMIN) or d > f32(VMAX).  A NaN is in neither set, both infinities are.
I24_HD bool i24_overflows(float d, const I24Par &p) { return d < p.vmin_f || d > p.vmax_f; }

// 376-378 with ALPHA = 1: every step a float32 operation rounded on its own, the division IEEE.  A NaN pixel gets code 0: numpy's cast of
// NaN to int32 is INT_MIN on x86-64 (where the fixtures are made) and the clip lifts it to 0.
I24_HD int i24_quantise(float d, const I24Par &p)
{
    if (d != d) return 0;
    const float c = d < p.vmin_f ? p.vmin_f : (d > p.vmax_f ? p.vmax_f : d);
    const float num = c - p.vmin_f;
#ifdef __HIP_DEVICE_COMPILE__
    const float y = __fdiv_rn(num, p.range_f);
#else
    const float y = num / p.range_f;
#endif
    const float f = floorf(p.scale_f * y);  // (a product with a power of two: exact)
    const int top = (1 << p.bitkeep) - 1;
    if (!(f > 0.0f)) return 0;  // (a NaN of 0 / 0 too)
    return f >= (float)top ? top : (int)f;
}

// 150-154: (q - qprev) mod 2^B.
I24_HD int i24_diff_fwd(int q, int qprev, int bitkeep) { return (int)(((uint32_t)q - (uint32_t)qprev) & ((1u << bitkeep) - 1u)); }

// 383 (s > 0) and 212 (s == -1); any other s does nothing.
I24_HD int i24_softbias_fwd(int q, int bitkeep, int s)
{
    if (s > 0) return (int)(((uint32_t)s + (uint32_t)q) & ((1u << bitkeep) - 1u));
    if (s == -1) return q >= (1 << (bitkeep - 1)) ? 2 * ((1 << bitkeep) - q) - 1 : 2 * q;
    return q;
}

// 409 (s > 0) and 237 (s == -1) in numpy's int32: wrapping sums, the floor modulus by a power of two, the floor division by two.
I24_HD int i24_softbias_rev(int q, int bitkeep, int s)
{
    if (s > 0) return (int)(((1u << bitkeep) - (uint32_t)s + (uint32_t)q) & ((1u << bitkeep) - 1u));
    if (s == -1) return (q & 1) ? (int)((1u << bitkeep) - 1u - (uint32_t)(q >> 1)) : (q >> 1);
    return q;
}

// 414-415 with ALPHA = 1: y = (0.5 + q) / 2^B is exact in float64; the product and the sum are rounded separately (no fused
// multiply-add may form), then one cast.
I24_HD float i24_dequantise(int q, const I24Par &p)
{
    const double y = (0.5 + (double)q) / (double)(1 << p.bitkeep);
#ifdef __HIP_DEVICE_COMPILE__
    return (float)__dadd_rn(p.vmin, __dmul_rn(p.range, y));
#else
    volatile double prod = p.range * y;
    return (float)(p.vmin + prod);
#endif
}

// ---- the bit stream of REORDER ---------------------------------------------------------------------------------------------------------
// Plane j of a layer of n pixels is a stream of 8 n bits: stream bit s is bit s / n of the plane's byte of pixel s % n, and bit t of output
// byte k is stream bit 8 k + t.

I24_HD long i24_stream_pos(long pixel, int bit, long n) { return (long)bit * n + pixel; }

// The output bytes of bit `b` that the tile of pixels [p0, p1) owns: byte k belongs to the tile that holds the pixel of its first stream
// bit, so k0 <= k < k1 with 8 k in [b n + p0, b n + p1).  Every byte of the plane has exactly one owner; a tile owns at most I24_THREADS
// bytes of one bit.
I24_HD void i24_tile_bytes(long n, long p0, long p1, int b, long *k0, long *k1)
{
    const long s0 = (long)b * n + p0, s1 = (long)b * n + p1;
    *k0 = (s0 + 7) >> 3;
    *k1 = (s1 + 7) >> 3;
}

// Output byte k of every plane, gathered by its owner (plane j's byte in bits 8 j .. 8 j + 7 of the result): code_at(pixel) is the pixel's
// transformed code.  The first stream bit is bit b of pixel pf = 8 k - b n; the following ones run on to pixel pf + 7 and, past the last
// pixel, into the next bit from pixel 0 (with n < 8 more than once).
template <typename F>
I24_HD uint32_t i24_gather_planes(long k, long n, F code_at)
{
    int b = (int)((8 * k) / n);
    long q = 8 * k - (long)b * n;
    uint32_t out = 0;
    for (int t = 0; t < 8; t++) {
        while (q >= n) q -= n, b++;
        const uint32_t c = (uint32_t)code_at(q) >> b;
        out |= ((c & 1u) | ((c >> 8 & 1u) << 8) | ((c >> 16 & 1u) << 16)) << t;
        q++;
    }
    return out;
}

// The plane's byte of pixel p back from the stream (lsbf_rev): bit b is stream bit b n + p.  byte_at(k) is output byte k of the plane.
template <typename F>
I24_HD unsigned i24_scatter_byte(long p, long n, F byte_at)
{
    unsigned out = 0;
    for (int b = 0; b < 8; b++) {
        const long s = i24_stream_pos(p, b, n);
        out |= (((unsigned)byte_at(s >> 3) >> (s & 7)) & 1u) << b;
    }
    return out;
}

// ---- the ranking of a tile's overflow hits -------------------------------------------------------------------------------------------
// Thread t looks at pixels p0 + i I24_THREADS + t, i = 0 .. I24_ITEMS - 1.  The hits of (item i, wave w) are slot i I24_WAVES + w; in
// ascending flat order the slots come in ascending slot number and inside a slot the lanes ascend.  A hit's rank in its tile is the
// number of hits in lower slots plus the number among the lower lanes of its own ballot.
I24_HD long i24_rank_pixel(long p0, int item, int thread) { return p0 + (long)item * I24_THREADS + thread; }
I24_HD int i24_rank_slot(int item, int wave) { return item * I24_WAVES + wave; }

// counts[I24_SLOTS] -> their exclusive prefix sums in place; returns the tile's total.
I24_HD unsigned i24_slot_offsets(unsigned *counts)
{
    unsigned run = 0;
    for (int s = 0; s < I24_SLOTS; s++) {
        const unsigned c = counts[s];
        counts[s] = run;
        run += c;
    }
    return run;
}

I24_HD int i24_popcount_below(uint64_t ballot, int lane) { uint64_t m = ballot & ((1ull << lane) - 1ull); int c = 0; while (m) { m &= m - 1; c++; } return c; }

// ---- the prefix sum -------------------------------------------------------------------------------------------------------------------
// In the scan thread t holds the I24_ITEMS consecutive pixels p0 + t I24_ITEMS + e.  The inclusive prefix of pixel (t, e) is the tile's
// base + the sum of the threads below t + the thread's own running sum; all in wrapping 32-bit arithmetic (2^BITKEEP divides 2^32).
I24_HD long i24_scan_pixel(long p0, int thread, int e) { return p0 + (long)thread * I24_ITEMS + e; }

// The tile sums [ntiles] of one layer -> their exclusive prefix sums in place, taken I24_SCAN_CHUNK at a time with a carry, as the one
// workgroup of the middle launch walks them (`step(chunk, count, carry)` scans one chunk exclusively from `carry` and returns the new
// carry); returns the layer's total.
template <typename F>
I24_HD uint32_t i24_scan_chunks(uint32_t *sums, long ntiles, F step)
{
    uint32_t carry = 0;
    for (long c0 = 0; c0 < ntiles; c0 += I24_SCAN_CHUNK) {
        const long cnt = ntiles - c0 < I24_SCAN_CHUNK ? ntiles - c0 : I24_SCAN_CHUNK;
        carry = step(sums + c0, (int)cnt, carry);
    }
    return carry;
}

}  // namespace imcom
