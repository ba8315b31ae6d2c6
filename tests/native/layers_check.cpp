// layers_check.cpp -- the host-compilable core of imcom_layer_place (pyimcom_amd/csrc/layers_core.h) against plain loops, under the
// sanitizers (tests/test_layercube_host.py builds and runs it).  For every element type, byte order, flip, crop origin, subtraction and
// rescale, at the golden's side (24) and at 1, 63, 64, 65 and 257: the plane formed pixel by pixel through layer_src_index / layer_value
// equals the plane formed the way the reference does it -- take the window, assign it (minus the sky) to a float32 plane, reverse the plane,
// multiply it.  Sources live in heap blocks of exactly their size, so an index that leaves one is an AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "layers_core.h"

using namespace imcom;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    uint64_t x = rng_state;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 29;
    return x;
}

// element k of a source of `type` as native bytes: a spread of magnitudes, with NaN, the infinities and -0.0 among the floats
static void native_element(int type, long k, unsigned char *out)
{
    const uint64_t r = next_u64();
    const double mag = std::ldexp((double)(r >> 11) / 9007199254740992.0 - 0.5, (int)(r % 40) - 10);
    switch (type) {
    case LAYER_F32: {
        float v = (float)(86.0 + mag);
        if (k % 97 == 5) v = NAN;
        if (k % 97 == 6) v = INFINITY;
        if (k % 97 == 7) v = -INFINITY;
        if (k % 97 == 8) v = -0.0f;
        memcpy(out, &v, 4);
        break;
    }
    case LAYER_F64: {
        double v = 86.0 + mag * 1.000000123;
        if (k % 97 == 5) v = NAN;
        if (k % 97 == 6) v = INFINITY;
        if (k % 97 == 7) v = -INFINITY;
        if (k % 97 == 8) v = -0.0;
        if (k % 97 == 9) v = 1.0e300;  // rounds to infinity in float32
        memcpy(out, &v, 8);
        break;
    }
    case LAYER_I16: { int16_t v = (int16_t)(r >> 20); memcpy(out, &v, 2); break; }
    case LAYER_U16: { uint16_t v = (uint16_t)(r >> 20); memcpy(out, &v, 2); break; }
    case LAYER_I32: { int32_t v = (int32_t)(r >> 16); memcpy(out, &v, 4); break; }
    default: out[0] = (unsigned char)(r >> 30);
    }
}

static double native_as_double(int type, const unsigned char *p, float *as_f32)
{
    switch (type) {
    case LAYER_F32: memcpy(as_f32, p, 4); return (double)*as_f32;
    case LAYER_F64: { double v; memcpy(&v, p, 8); return v; }
    case LAYER_I16: { int16_t v; memcpy(&v, p, 2); return (double)v; }
    case LAYER_U16: { uint16_t v; memcpy(&v, p, 2); return (double)v; }
    case LAYER_I32: { int32_t v; memcpy(&v, p, 4); return (double)v; }
    default: return (double)p[0];
    }
}

static bool same_bits(float a, float b)
{
    uint32_t ua, ub;
    memcpy(&ua, &a, 4);
    memcpy(&ub, &b, 4);
    return ua == ub || (a != a && b != b);
}

template <int TYPE>
static float core_value(const void *src, long idx, int swapped, int op, double sub, int ps, double scale)
{
    return layer_value<TYPE>(src, idx, swapped, op, sub, ps, scale);
}

static float dispatch(int type, const void *src, long idx, int swapped, int op, double sub, int ps, double scale)
{
    switch (type) {
    case LAYER_F32: return core_value<LAYER_F32>(src, idx, swapped, op, sub, ps, scale);
    case LAYER_F64: return core_value<LAYER_F64>(src, idx, swapped, op, sub, ps, scale);
    case LAYER_I16: return core_value<LAYER_I16>(src, idx, swapped, op, sub, ps, scale);
    case LAYER_U16: return core_value<LAYER_U16>(src, idx, swapped, op, sub, ps, scale);
    case LAYER_I32: return core_value<LAYER_I32>(src, idx, swapped, op, sub, ps, scale);
    default: return core_value<LAYER_U8>(src, idx, swapped, op, sub, ps, scale);
    }
}

int main()
{
    long planes = 0, pixels = 0, bad = 0;
    const int sides[] = {24, 1, 63, 64, 65, 257};
    const double sub = 86.123456789, scales[] = {2.5, 0.1};
    for (int nside : sides)
        for (int type = 0; type < LAYER_NTYPES; type++)
            for (int swapped = 0; swapped < 2; swapped++)
                for (int crop = 0; crop < 3; crop++) {  // the whole source; origin (4, 4) of a source 4 or 8 wider
                    const int esz = layer_type_size(type), ny = nside + (crop == 0 ? 0 : crop == 1 ? 4 : 8), nx = ny, y0 = crop ? 4 : 0, x0 = y0;
                    // the native values, and the bytes as the file holds them (reversed per element when swapped), in an exact-size block
                    std::vector<unsigned char> native((size_t)ny * nx * esz);
                    for (long k = 0; k < (long)ny * nx; k++) native_element(type, k, &native[(size_t)k * esz]);
                    unsigned char *file = (unsigned char *)malloc((size_t)ny * nx * esz);
                    for (long k = 0; k < (long)ny * nx; k++)
                        for (int b = 0; b < esz; b++) file[(size_t)k * esz + b] = native[(size_t)k * esz + (swapped ? esz - 1 - b : b)];
                    if (layer_place_check(type, swapped, ny, nx, y0, x0, 0, 0, 0, nside) != 0) bad++;
                    for (int flip = 0; flip < 3; flip++)
                        for (int op = 0; op < 2; op++)
                            for (int ps = 0; ps < 3; ps++) {
                                const double scale = ps ? scales[ps - 1] : 0.0;
                                // the reference's way: window -> plane (minus the sky) -> reversed plane -> times rescale
                                std::vector<float> plane((size_t)nside * nside), want((size_t)nside * nside);
                                for (int y = 0; y < nside; y++)
                                    for (int x = 0; x < nside; x++) {
                                        float f = 0.0f;
                                        const double d = native_as_double(type, &native[((size_t)(y0 + y) * nx + (x0 + x)) * esz], &f);
                                        float v;
                                        if (type == LAYER_F32) v = op ? f - (float)sub : f;
                                        else v = (float)(op ? d - sub : d);
                                        plane[(size_t)y * nside + x] = v;
                                    }
                                for (int y = 0; y < nside; y++)
                                    for (int x = 0; x < nside; x++) {
                                        const int sy = flip == 2 ? nside - 1 - y : y, sx = flip == 1 ? nside - 1 - x : x;
                                        float v = plane[(size_t)sy * nside + sx];
                                        if (ps) v = v * (float)scale;
                                        want[(size_t)y * nside + x] = v;
                                    }
                                for (int y = 0; y < nside; y++)
                                    for (int x = 0; x < nside; x++) {
                                        const long idx = layer_src_index(y, x, nside, flip, y0, x0, nx);
                                        const float got = dispatch(type, file, idx, swapped, op, sub, ps ? 1 : 0, scale);
                                        if (!same_bits(got, want[(size_t)y * nside + x])) bad++;
                                        pixels++;
                                    }
                                planes++;
                            }
                    free(file);
                }
    // the literal slice [4:4092] of an axis of n elements
    const long ns[] = {0, 3, 4, 5, 24, 28, 32, 4088, 4091, 4092, 4093, 4096, 5000}, ext[] = {0, 0, 0, 1, 20, 24, 28, 4084, 4087, 4088, 4088, 4088, 4088};
    long extents = 0;
    for (int k = 0; k < 13; k++, extents++)
        if (layer_crop_extent(ns[k]) != ext[k]) bad++;
    // the swaps are involutions that reverse the bytes
    if (layer_bswap16(0x1234) != 0x3412 || layer_bswap32(0x12345678u) != 0x78563412u || layer_bswap64(0x0102030405060708ull) != 0x0807060504030201ull) bad++;
    // refusals: each rule once
    long refusals = 0;
    const int want_rule[] = {1, 1, 2, 2, 3, 3, 4, 5, 5, 5, 6, 6, 6, 6, 0, 0};
    const int got_rule[] = {layer_place_check(-1, 0, 8, 8, 0, 0, 0, 0, 0, 8), layer_place_check(6, 0, 8, 8, 0, 0, 0, 0, 0, 8), layer_place_check(0, 2, 8, 8, 0, 0, 0, 0, 0, 8),
                            layer_place_check(0, 0, 8, 8, 0, 0, 0, 0, -1, 8), layer_place_check(0, 0, 8, 8, 0, 0, 3, 0, 0, 8), layer_place_check(0, 0, 8, 8, 0, 0, -1, 0, 0, 8),
                            layer_place_check(0, 0, 8, 8, 0, 0, 0, 2, 0, 8), layer_place_check(0, 0, 8, 8, 0, 0, 0, 0, 0, -1), layer_place_check(0, 0, -8, 8, 0, 0, 0, 0, 0, 8),
                            layer_place_check(0, 0, 8, 65537, 0, 0, 0, 0, 0, 8), layer_place_check(0, 0, 8, 8, -1, 0, 0, 0, 0, 8), layer_place_check(0, 0, 8, 8, 0, 1, 0, 0, 0, 8),
                            layer_place_check(0, 0, 11, 12, 4, 4, 0, 0, 0, 8), layer_place_check(0, 0, 12, 11, 4, 4, 0, 0, 0, 8), layer_place_check(0, 0, 12, 12, 4, 4, 0, 0, 0, 8),
                            layer_place_check(5, 1, 0, 0, 0, 0, 2, 1, 1, 0)};
    for (int k = 0; k < 16; k++, refusals++)
        if (got_rule[k] != want_rule[k]) bad++;
    printf("planes %ld\npixels %ld\nextents %ld\nrefusals %ld\nmismatches %ld\n", planes, pixels, extents, refusals, bad);
    return bad ? 1 : 0;
}
