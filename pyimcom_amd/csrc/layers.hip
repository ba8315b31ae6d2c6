// layers.hip -- one plane of the input-layer cube (reference src/pyimcom/layer.py:1199-1527, get_all_data): every plane that no generator
// writes -- the science frame minus its sky (1261), truth (1284-1295), labnoise and its literal crop (1322-1335), skyerr (1344), a saved
// noise slice (1484), and the float64 images of the white-noise and star-grid seams on their way into the float32 cube (1304, 1351) -- is
// `plane = flip(window(source)) [- sky] [* rescale]` of a source of one of six element types in either byte order.  A FITS image arrives
// as the file's big-endian bytes and is swapped here: the host makes no pass over it.
//
// One thread owns one output pixel: no atomics, and every result has one value.  Consecutive threads own consecutive x: the stores of a
// wave are one run of the row, and so are its loads -- for the x flip the same run read backwards, which the memory system serves as the
// same lines.  The kernel moves element-size + 4 bytes a pixel and does nothing else; the per-pixel code is layers_core.h.  The C entry
// imcom_layer_place stands beside imcom_extract_layers (partition.hip), the cube's consumer.
#include "launchers.h"
#include "layers_core.h"

namespace imcom {

template <int TYPE>
__global__ __launch_bounds__(256) void layer_place_kernel(const void *__restrict__ src, int swapped, int src_nx, int y0, int x0, int flip, int op, double sub,
                                                          int post_scale_flag, double scale, float *__restrict__ dst, int nside)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)nside * nside) return;
    const int y = (int)(i / nside), x = (int)(i - (long)y * nside);
    dst[i] = layer_value<TYPE>(src, layer_src_index(y, x, nside, flip, y0, x0, src_nx), swapped, op, sub, post_scale_flag, scale);
}

// src [src_ny, src_nx] and dst [nside, nside] are device memory; the arguments have passed layer_place_check and nside >= 1.
int launch_layer_place(imcom_ctx *ctx, const void *src, int src_type, int src_swapped, int src_nx, int y0, int x0, int flip, int op, double sub, int post_scale_flag,
                       double scale, float *dst, int nside)
{
    ProfScope ps(ctx, "layer_place");
    const dim3 grid((unsigned)(((long)nside * nside + 255) / 256)), block(256);
#define IMCOM_LAYER_CASE(T)                                                                                                                              \
    case T:                                                                                                                                              \
        hipLaunchKernelGGL(layer_place_kernel<T>, grid, block, 0, ctx->stream, src, src_swapped, src_nx, y0, x0, flip, op, sub, post_scale_flag, scale, \
                           dst, nside);                                                                                                                  \
        break;
    switch (src_type) {
        IMCOM_LAYER_CASE(LAYER_F32)
        IMCOM_LAYER_CASE(LAYER_F64)
        IMCOM_LAYER_CASE(LAYER_I16)
        IMCOM_LAYER_CASE(LAYER_U16)
        IMCOM_LAYER_CASE(LAYER_I32)
        IMCOM_LAYER_CASE(LAYER_U8)
    default:
        set_error("layer_place: source type %d", src_type);
        return IMCOM_ERR_ARG;
    }
#undef IMCOM_LAYER_CASE
    return check_launch("layer_place_kernel");
}

}  // namespace imcom
