// objmask_core.h -- the arithmetic of objmask.hip that has one right answer and no device in it: the order-preserving integer keys of the
// exact selection, its digit schedule, and one row step of the constrained flood.  Compiles as host code too (tests/native/objmask_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define OM_HD __host__ __device__ __forceinline__
#else
#define OM_HD inline
#endif

namespace imcom {

// Keys: a < b as numbers <=> key(a) < key(b) as unsigned integers, for every pair that is not NaN; -0.0 and 0.0 share the key of 0.0.
// (Sign bit set: all bits flipped; clear: the sign bit set.)  A NaN has no key: the caller counts it.
OM_HD uint64_t om_key(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000u) ? (uint32_t)~u : (u | 0x80000000u);
}
OM_HD uint64_t om_key(double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    if ((u << 1) == 0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
OM_HD float om_value_f32(uint64_t key)
{
    const uint32_t k = (uint32_t)key, u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
OM_HD double om_value_f64(uint64_t key)
{
    const uint64_t u = (key >> 63) ? (key ^ 0x8000000000000000ull) : ~key;
    double v;
    memcpy(&v, &u, 8);
    return v;
}

// The digits, from the top: 11 / 11 / 10 bits of a 32-bit key, 11 x 5 + 9 of a 64-bit key.
constexpr int OM_DIGIT_BITS = 11, OM_BINS = 1 << OM_DIGIT_BITS;
OM_HD int om_passes(int keybits) { return keybits == 32 ? 3 : 6; }
OM_HD void om_digit(int keybits, int pass, int *shift, int *nbits)
{
    const int top = keybits - OM_DIGIT_BITS * pass;  // bits not yet decided
    *nbits = top < OM_DIGIT_BITS ? top : OM_DIGIT_BITS;
    *shift = top - *nbits;
}

// One row of the flood: `s` the row's set pixels, `up` / `down` those of the rows above and below, `g` the row's grow pixels, a bit per
// column.  The row takes what its vertical neighbours hand to its grow pixels and then spreads along itself through grow pixels until
// nothing moves (at most 64 rounds).  Set pixels outside `g` stay set and spread like any other.
OM_HD uint64_t om_flood_row(uint64_t s, uint64_t up, uint64_t down, uint64_t g)
{
    uint64_t n = s | ((up | down) & g), p;
    do {
        p = n;
        n |= ((n << 1) | (n >> 1)) & g;
    } while (n != p);
    return n;
}

}  // namespace imcom
