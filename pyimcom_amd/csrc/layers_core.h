// layers_core.h -- the per-pixel part of imcom_layer_place (layers.hip), the placement of one source image into a plane of the input-layer
// cube (reference src/pyimcom/layer.py:1199-1527, get_all_data): the element types, the byte swap, the index map (crop origin, the extent
// of the literal slice [4:4092], the two flips of 1287-1290 / 1332-1335) and numpy's arithmetic of `plane = data - sky` and `plane *= rescale`.
// Plain C++ that compiles as host code as it stands (tests/native/layers_check.cpp walks it against plain loops) and as device code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LAYERS_HD __host__ __device__ __forceinline__
#else
#define LAYERS_HD inline
#endif

namespace imcom {

// src_type of imcom_layer_place: the numpy dtypes a FITS or ASDF image comes in
enum { LAYER_F32 = 0, LAYER_F64 = 1, LAYER_I16 = 2, LAYER_U16 = 3, LAYER_I32 = 4, LAYER_U8 = 5, LAYER_NTYPES = 6 };
enum { LAYER_FLIP_NONE = 0, LAYER_FLIP_X = 1, LAYER_FLIP_Y = 2 };
enum { LAYER_OP_NONE = 0, LAYER_OP_SUBTRACT = 1 };
constexpr long LAYER_MAX_SIDE = 65536;

LAYERS_HD int layer_type_size(int type)
{
    switch (type) {
    case LAYER_F32: return 4;
    case LAYER_F64: return 8;
    case LAYER_I16: return 2;
    case LAYER_U16: return 2;
    case LAYER_I32: return 4;
    case LAYER_U8: return 1;
    default: return 0;
    }
}

LAYERS_HD uint16_t layer_bswap16(uint16_t v) { return (uint16_t)((v >> 8) | (v << 8)); }
LAYERS_HD uint32_t layer_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0x0000FF00u) | ((v << 8) & 0x00FF0000u) | (v << 24); }
LAYERS_HD uint64_t layer_bswap64(uint64_t v) { return ((uint64_t)layer_bswap32((uint32_t)v) << 32) | (uint64_t)layer_bswap32((uint32_t)(v >> 32)); }

// The length of the slice [4:4092] of an axis of n elements, as Python forms it (layer.py:1324).
LAYERS_HD long layer_crop_extent(long n)
{
    const long stop = n < 4092 ? n : 4092;
    return stop > 4 ? stop - 4 : 0;
}

// Where output pixel (y, x) of the plane [nside, nside] reads its source [src_ny, src_nx]: the window of origin (y0, x0), reversed along x
// (`plane[:, ::-1]`, SCAs 3, 6, ...) or along y (`plane[::-1, :]`).
LAYERS_HD long layer_src_index(int y, int x, int nside, int flip, int y0, int x0, int src_nx)
{
    const int sy = flip == LAYER_FLIP_Y ? nside - 1 - y : y, sx = flip == LAYER_FLIP_X ? nside - 1 - x : x;
    return (long)(y0 + sy) * src_nx + (x0 + sx);
}

// 0 when the arguments describe a placement that stays inside the source; else the number of the first rule broken (the entry's message).
LAYERS_HD int layer_place_check(int src_type, int src_swapped, long src_ny, long src_nx, long y0, long x0, int flip, int op, int post_scale_flag, long nside)
{
    if (src_type < 0 || src_type >= LAYER_NTYPES) return 1;
    if (src_swapped < 0 || src_swapped > 1 || post_scale_flag < 0 || post_scale_flag > 1) return 2;
    if (flip < LAYER_FLIP_NONE || flip > LAYER_FLIP_Y) return 3;
    if (op < LAYER_OP_NONE || op > LAYER_OP_SUBTRACT) return 4;
    if (nside < 0 || nside > LAYER_MAX_SIDE || src_ny < 0 || src_ny > LAYER_MAX_SIDE || src_nx < 0 || src_nx > LAYER_MAX_SIDE) return 5;
    if (y0 < 0 || x0 < 0 || y0 + nside > src_ny || x0 + nside > src_nx) return 6;
    return 0;
}

// Element idx of the source as numpy reads it: the bytes in the file's order when src_swapped, in the machine's otherwise.
template <int TYPE>
LAYERS_HD float layer_load_f32(const void *src, long idx, int swapped)
{
    uint32_t u = ((const uint32_t *)src)[idx];
    if (swapped) u = layer_bswap32(u);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

template <int TYPE>
LAYERS_HD double layer_load_f64(const void *src, long idx, int swapped)  // exact for every type but LAYER_F32's own path above
{
    if (TYPE == LAYER_F64) {
        uint64_t u = ((const uint64_t *)src)[idx];
        if (swapped) u = layer_bswap64(u);
        double d;
        __builtin_memcpy(&d, &u, 8);
        return d;
    }
    if (TYPE == LAYER_I16 || TYPE == LAYER_U16) {
        uint16_t u = ((const uint16_t *)src)[idx];
        if (swapped) u = layer_bswap16(u);
        return TYPE == LAYER_I16 ? (double)(int16_t)u : (double)u;
    }
    if (TYPE == LAYER_I32) {
        uint32_t u = ((const uint32_t *)src)[idx];
        if (swapped) u = layer_bswap32(u);
        return (double)(int32_t)u;
    }
    return (double)((const uint8_t *)src)[idx];
}

// numpy >= 2 on `plane[...] = data - float(sky)` and `plane *= rescale` with a float32 plane: a float32 image stays float32 against the
// Python float (both operands float32, one rounding); a float64 or integer image is promoted to float64, the difference is formed
// there and the assignment rounds it to float32 (to nearest even); the product is float32 by float32(rescale).  Nothing here is of the
// form a * b + c, so no contraction can change a bit.
template <int TYPE>
LAYERS_HD float layer_value(const void *src, long idx, int swapped, int op, double sub, int post_scale_flag, double scale)
{
    float v;
    if (TYPE == LAYER_F32) {
        v = layer_load_f32<TYPE>(src, idx, swapped);
        if (op == LAYER_OP_SUBTRACT) v = v - (float)sub;
    } else {
        double d = layer_load_f64<TYPE>(src, idx, swapped);
        if (op == LAYER_OP_SUBTRACT) d = d - sub;
        v = (float)d;
    }
    if (post_scale_flag) v = v * (float)scale;
    return v;
}

}  // namespace imcom
