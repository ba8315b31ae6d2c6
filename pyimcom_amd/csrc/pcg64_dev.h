// pcg64_dev.h -- device pieces of numpy's PCG64 stream shared by pcg64.hip and ziggurat.hip: the 128-bit affine step, the jump table of a
// call in LDS, the jump over d steps and one step with its 64-bit output.
#pragma once
#include "launchers.h"

namespace imcom {

struct U128 {
    unsigned long long lo, hi;
};

// a s + c mod 2^128, in 64-bit halves
__device__ __forceinline__ U128 affine(const U128 a, const U128 s, const U128 c)
{
    U128 r;
    r.lo = a.lo * s.lo;
    r.hi = __umul64hi(a.lo, s.lo) + a.lo * s.hi + a.hi * s.lo;
    r.lo += c.lo;
    r.hi += c.hi + (r.lo < c.lo);
    return r;
}

// the jump table of a call, [PCG64_JUMPS][2] (A_j, C_j), from global memory into LDS (4 KB); the caller synchronises
__device__ __forceinline__ void load_jumps(U128 *tab, const unsigned long long *__restrict__ jumps)
{
    for (int i = threadIdx.x; i < 2 * PCG64_JUMPS; i += blockDim.x) {
        tab[i].lo = jumps[2 * i];
        tab[i].hi = jumps[2 * i + 1];
    }
}

// the state d steps after s, d = dhi 2^64 + dlo
__device__ __forceinline__ U128 jump(U128 s, unsigned long long dlo, unsigned long long dhi, const U128 *tab)
{
    for (int j = 0; (dlo | dhi) != 0; j++) {
        if (dlo & 1) s = affine(tab[2 * j], s, tab[2 * j + 1]);
        dlo = (dlo >> 1) | (dhi << 63);
        dhi >>= 1;
    }
    return s;
}

// one step; the 64-bit output of the new state
__device__ __forceinline__ unsigned long long step_output(U128 &s, const U128 *tab)
{
    s = affine(tab[0], s, tab[1]);
    const unsigned long long x = s.hi ^ s.lo;
    const unsigned rot = (unsigned)(s.hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));  // (rot = 0: both shifts are by 0)
}

}  // namespace imcom
