// padshare_core.h -- the arithmetic of sharing padding stamps between neighbouring blocks (seam 20; reference src/pyimcom/analysis.py
// OutImage._update_hdu_data 394-537 and get_output_map 344-392) that has one right answer and no device in it: the strip of "my" block
// that a call writes and the strip of the neighbour it reads (435-446, 472-483, 506-528), the taper index of a strip position on either
// side (OutStamp.trapezoid, coadd.py:1222-1292, with the pad widths of 504-526), the decode of a coded quality map value (377-387), the
// combine `mine * add_mode + theirs` (448-450, 535) and the encode of Block.compress_map (coadd.py:2123-2130) as compress_map_kernel
// forms it.  Every float32 product and sum is rounded on its own: no contraction.  Compiles as host code too
// (tests/native/padshare_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif

namespace imcom {

enum { PS_LEFT = 0, PS_RIGHT = 1, PS_BOTTOM = 2, PS_TOP = 3 };
constexpr int PS_NO_FLOOR = 1 << 20;  // a floor code no (u)int16 takes: zero nothing

PS_HD bool ps_along_x(int direction) { return direction < PS_BOTTOM; }  // left / right: the strip is a range of columns; else of rows
PS_HD bool ps_low(int direction) { return (direction & 1) == 0; }       // left / bottom: my strip starts at index 0

// The strips along the axis that `direction` names, for a side of n pixels, a padding region of w and a fade kernel fk (435-446;
// INWEIGHT, 472-483, is the same with n = n1P, w = postage_pad, fk = 0): positions p = 0 .. len - 1 are my0 + p of mine, ur0 + p of theirs.
struct PsStrip {
    int my0, ur0, len;
};
PS_HD PsStrip ps_strip(int direction, int n, int w, int fk)
{
    PsStrip s;
    s.len = w + fk;
    if (ps_low(direction)) { s.my0 = 0; s.ur0 = n - 2 * w; }
    else { s.my0 = n - w - fk; s.ur0 = w - fk; }
    return s;
}
// What every entry checks before it trusts ps_strip: both strips lie inside 0 .. n - 1.
PS_HD bool ps_shape_ok(int direction, int n, int w, int fk)
{
    return direction >= PS_LEFT && direction <= PS_TOP && n >= 1 && fk >= 0 && w >= fk && 2L * w <= n;
}

// The taper index k (0 .. 2 fk - 1; the weight is s_{k+1}) of strip position p in add mode, -1 where the value is not tapered.  My map
// is tapered on the side that is updated with pad width w - fk, the neighbour's on the opposite side (504-526): on the low side my
// fade rises over p = w - fk .. w + fk - 1 while the neighbour's falls, on the high side mine falls over p = 0 .. 2 fk - 1.
PS_HD int ps_taper_mine(int direction, int p, int w, int fk)
{
    if (ps_low(direction)) return p >= w - fk ? p - (w - fk) : -1;
    return p < 2 * fk ? 2 * fk - 1 - p : -1;
}
PS_HD int ps_taper_theirs(int direction, int p, int w, int fk)
{
    if (ps_low(direction)) return p >= w - fk ? w + fk - 1 - p : -1;
    return p < 2 * fk ? p : -1;
}
// coadd.py:1269-1271 and numpy's in-place float32 *= float64: one product in double, rounded to float32.
PS_HD float ps_taper(float v, int k, int fk)
{
    if (k < 0) return v;
    double s = (double)(k + 1) / (2 * fk + 1);
    s -= sin(6.283185307179586 * s) / 6.283185307179586;
    return (float)((double)v * s);
}

// A code as a number, from the two's complement bits that serve both int16 and uint16.
PS_HD int ps_code(uint16_t bits, int is_unsigned) { return is_unsigned ? (int)bits : (int)(int16_t)bits; }
// get_output_map 377-387: float32(10 ** (code / coef)) with coef the double 1 / HDU_to_bels; the floor code (or PS_NO_FLOOR) gives 0.
PS_HD float ps_decode(int code, double coef, int floor_code)
{
    if (code == floor_code) return 0.0f;
    return (float)pow(10.0, (double)code / coef);
}

// mine * add_mode + theirs in float32 (the product by the bool is formed: -0.0 * False + 0.0 = +0.0, inf * False = NaN).
PS_HD float ps_combine(float mine, float theirs, int add_mode)
{
    const float m = add_mode ? 1.0f : 0.0f;
#ifdef __HIP_DEVICE_COMPILE__
    return __fadd_rn(__fmul_rn(mine, m), theirs);
#else
    volatile float p = mine * m;  // (rounded to float32 before the sum, whatever the host's evaluation method)
    return p + theirs;
#endif
}

// Block.compress_map: clip(floor(coef * log10(clip(v, 1e-32, None)) + 0.5), a_min, a_max) in float32 with a correctly rounded log10
// (computed in double); NaN gives a_min.  Returns the two's complement bits.
PS_HD uint16_t ps_encode(float v, float coef, int is_unsigned)
{
    const float a_min = is_unsigned ? 0.0f : -32768.0f, a_max = is_unsigned ? 65535.0f : 32767.0f;
    const float x = fmaxf(v, 1e-32f);
    const float l = (float)log10((double)x);
#ifdef __HIP_DEVICE_COMPILE__
    float c = floorf(__fadd_rn(__fmul_rn(coef, l), 0.5f));
#else
    volatile float p = coef * l;
    volatile float q = p + 0.5f;
    float c = floorf(q);
#endif
    c = fminf(fmaxf(c, a_min), a_max);
    if (!(c == c)) c = a_min;
    return (uint16_t)((int)c & 0xffff);
}

}  // namespace imcom
