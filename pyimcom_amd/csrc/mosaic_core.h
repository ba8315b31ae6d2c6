// mosaic_core.h -- the statements of the metadetection mosaic (seam 19; reference src/pyimcom/meta/distortimage.py) that have one right
// answer and no device in them: where a row of a block's window lies in the block file and in the mosaic (193-207), how such a row is cut
// into 16-byte pieces and scalar edges, the coded FIDELITY / SIGMA value in dB as numpy forms it in float32 (197-207), the box of a masked
// circle (341-344), the pixel a flat index of the boxes names, and the circle's predicate (352).  Compiles as host code too
// (tests/native/mosaic_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define MO_HD __host__ __device__ __forceinline__
#else
#define MO_HD inline
#endif

namespace imcom {

// The window of one block (distortimage.py:146-170): rows symin .. symax - 1 and columns sxmin .. sxmax - 1 of the block file go to the
// rows cy + symin .. and the columns cx + sxmin .. of the mosaic.
struct MoWindow {
    int symin, symax, sxmin, sxmax, cy, cx;
};
MO_HD int mo_rows(const MoWindow &W) { return W.symax - W.symin; }
MO_HD int mo_cols(const MoWindow &W) { return W.sxmax - W.sxmin; }
// Element offset of column 0 of window row r: in a block-file plane of row pitch `pitch`, in a mosaic plane of side ns.
MO_HD long mo_src_offset(const MoWindow &W, int r, long pitch) { return (long)(W.symin + r) * pitch + W.sxmin; }
MO_HD long mo_dst_offset(const MoWindow &W, int r, int ns) { return (long)(W.symin + W.cy + r) * ns + (W.sxmin + W.cx); }
// The window lies inside a block file of by x bx pixels and inside the mosaic.
MO_HD bool mo_window_ok(const MoWindow &W, int by, int bx, int ns)
{
    return 0 <= W.symin && W.symin <= W.symax && W.symax <= by && 0 <= W.sxmin && W.sxmin <= W.sxmax && W.sxmax <= bx && (long)W.symin + W.cy >= 0 &&
           (long)W.symax + W.cy <= ns && (long)W.sxmin + W.cx >= 0 && (long)W.sxmax + W.cx <= ns;
}

// A row of w elements of es bytes (4 or 8) from byte address src to byte address dst, both multiples of es: the elements 0 .. *lead - 1
// go one by one, then *nvec pieces of 16 bytes that are 16-byte aligned on both sides, then the rest one by one.  Where source and
// destination differ in their offset within 16 bytes there is no such piece (*nvec = 0).
MO_HD void mo_row_split(uint64_t dst, uint64_t src, int w, int es, int *lead, int *nvec)
{
    const int per = 16 / es;
    int l = (int)(((16 - (dst & 15)) & 15) / (unsigned)es);
    if (l > w) l = w;
    *lead = l;
    *nvec = ((src + (uint64_t)l * es) & 15) == 0 ? (w - l) / per : 0;
}

// A coded map value in dB (197-207): numpy's float32 `code.astype(float32) * bels / d`, d = -0.1 (FIDELITY) or 0.1 (SIGMA): two correctly
// rounded float32 operations.  The device takes mo_db_dev (no reciprocal, no contraction); this one is the host's.
MO_HD float mo_code_value(const void *codes, int type, long i)  // type: 0 uint8, 1 uint16, 2 int16
{
    if (type == 0) return (float)((const uint8_t *)codes)[i];
    if (type == 1) return (float)((const uint16_t *)codes)[i];
    return (float)((const int16_t *)codes)[i];
}
MO_HD float mo_db(float code, float bels, float d)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(__fmul_rn(code, bels), d);
#else
    volatile float p = code * bels;  // (rounded to float32 before the division, whatever the host's evaluation method)
    return p / d;
#endif
}
constexpr float MO_FIDELITY_DIV = (float)(-0.1), MO_NOISE_DIV = (float)0.1;

// The box of a circle (341-344): columns x0 .. x0 + w - 1, rows y0 .. y0 + h - 1; w = 0 or h = 0: nothing (346-347).  Formed in float64
// and clamped to [0, ns] before the conversion, so that no position overflows an integer; a position or radius that is not finite gives
// the empty box (the binding refuses it before the call).
struct MoBox {
    int x0, y0, w, h;
};
MO_HD int mo_clamp_index(double v, int ns) { return v < 0.0 ? 0 : (v > (double)ns ? ns : (int)v); }
MO_HD MoBox mo_cap_box(double x, double y, double r, int ns)
{
    MoBox b = {0, 0, 0, 0};
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(r))) return b;
    const int xmin = mo_clamp_index(std::floor(x - r), ns), xmax = mo_clamp_index(std::ceil(x + r) + 1.0, ns);
    const int ymin = mo_clamp_index(std::floor(y - r), ns), ymax = mo_clamp_index(std::ceil(y + r) + 1.0, ns);
    if (xmax <= xmin || ymax <= ymin) return b;
    b.x0 = xmin; b.y0 = ymin; b.w = xmax - xmin; b.h = ymax - ymin;
    return b;
}
MO_HD long mo_box_pixels(const MoBox &b) { return (long)b.w * b.h; }
// Pixel k (row-major, 0 <= k < w h) of a box.
MO_HD void mo_box_pixel(const MoBox &b, long k, int *ix, int *iy)
{
    const unsigned q = (unsigned)k / (unsigned)b.w;
    *iy = b.y0 + (int)q;
    *ix = b.x0 + (int)((unsigned)k - q * (unsigned)b.w);
}
// (352)
MO_HD bool mo_cap_hit(int ix, int iy, double x, double y, double r) { return hypot((double)ix - x, (double)iy - y) < r; }

}  // namespace imcom
