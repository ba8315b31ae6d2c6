// block.hip -- block-level accumulation of finished stamps on the device.
//
// Replaces the map updates of Block._output_stamp_wrapper (reference src/pyimcom/coadd.py:1975-1993:
// out_map / UC / Sigma / kappa / Tsum / Neff maps += the stamp's n2f x n2f tile at
// rows (j_st-1)*n2 .., cols (i_st-1)*n2 .., neighbouring stamps overlapping by 2*fade pixels) and the
// boundary recovery of Block.build_output_file (coadd.py:2163-2181: OutStamp.trapezoid(..., recover_mode=True,
// pad_widths)).  All maps are float32 as in the reference (coadd.py:2031-2047); float64 per-stamp inputs
// (Tsum_inpix, Neff) are added in double and rounded once, as numpy's `f32 += f64` does.
#include "common.h"
#include "launchers.h"

namespace imcom {

template <typename SRC>
__global__ void block_accumulate_kernel(int npass, const int *__restrict__ list, const int *__restrict__ jst,
                                        const int *__restrict__ ist, int n2, int n2f, int nlayer,
                                        const SRC *__restrict__ src, float *__restrict__ dst, int nside)
{
    // grid: (pixels of one tile, stamps of this parity pass, layers)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n2f * n2f || (int)blockIdx.y >= npass) return;
    const int s = list[blockIdx.y], layer = blockIdx.z;
    const int r = t / n2f, c = t - r * n2f;
    const int row = (jst[s] - 1) * n2 + r, col = (ist[s] - 1) * n2 + c;
    float *d = dst + ((long)layer * nside + row) * nside + col;
    const SRC v = src[((long)s * nlayer + layer) * n2f * n2f + t];
    *d = (float)((double)*d + (double)v);
}

// Overlapping stamps, any visiting order (fade > 0).  A pixel of the block belongs to at most four stamps, one of each index
// parity (2 * fade <= n2).  Every stamp's tile is STORED -- in the dtype it arrives in -- into the layer of its parity
// (block_place_kernel; tiles of one parity never overlap, so nothing is summed there), and block_combine_kernel then adds a
// pixel's layers in the order in which the reference's loop meets their stamps (coadd.py:2056-2059: cells of 2 x 2 stamps from
// (j_st_min, i_st_min) on, row by row of cells; inside a cell dj outer, di inner), each addition rounded as numpy's
// `f32_map[...] += tile` rounds it.  The block's maps therefore do not depend on how the
// stamps were dealt to batches, passes or processes, and carry the reference's own rounding.
template <typename SRC>
__global__ void block_place_kernel(int batch, const int *__restrict__ jst, const int *__restrict__ ist, int n2, int n2f,
                                   int nlayer, const SRC *__restrict__ src, SRC *__restrict__ layers, int nside)
{
    // grid: (pixels of one tile, stamps, layers)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n2f * n2f || (int)blockIdx.y >= batch) return;
    const int s = blockIdx.y, layer = blockIdx.z;
    const int r = t / n2f, c = t - r * n2f;
    const int row = (jst[s] - 1) * n2 + r, col = (ist[s] - 1) * n2 + c;
    const int par = ((jst[s] & 1) << 1) | (ist[s] & 1);
    layers[(((long)par * nlayer + layer) * nside + row) * nside + col] = src[((long)s * nlayer + layer) * n2f * n2f + t];
}

template <typename SRC>
__global__ void block_combine_kernel(int n1P, int n2, int n2f, long nlayer, const SRC *__restrict__ layers,
                                     float *__restrict__ dst, int nside, int cells, int pj, int pi)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= nlayer * nside * nside) return;
    const int col = (int)(t % nside), row = (int)((t / nside) % nside);
    const long layer = t / ((long)nside * nside);
    // 1-based stamps covering a row: (j-1) n2 <= row <= (j-1) n2 + n2f - 1
    auto first = [&](int r) { const int lo = r - n2f + 1; return (lo <= 0 ? 0 : (lo + n2 - 1) / n2) + 1; };
    auto last = [&](int r) { const int hi = r / n2 + 1; return hi < n1P ? hi : n1P; };
    // the visiting order of the reference's loop as a sort key: cells of 2 x 2 stamps starting at (pj, pi), row by row of cells,
    // inside a cell dj outer, di inner (coadd.py:2056-2059); cells = 0: plain rows (j outer, i inner)
    int key[4], nk = 0;
    SRC val[4];
    for (int j = first(row); j <= last(row); j++)
        for (int i = first(col); i <= last(col); i++) {
            const int par = ((j & 1) << 1) | (i & 1);
            const int k = cells ? (((((j - pj) >> 1) + 1) * 32768 + (((i - pi) >> 1) + 1)) * 2 + ((j - pj) & 1)) * 2 + ((i - pi) & 1) : j * 32768 + i;
            int q = nk++;
            const SRC v = layers[(((long)par * nlayer + layer) * nside + row) * nside + col];
            while (q > 0 && key[q - 1] > k) { key[q] = key[q - 1]; val[q] = val[q - 1]; q--; }
            key[q] = k;
            val[q] = v;
        }
    float d = 0.0f;
    for (int q = 0; q < nk; q++) d = (float)((double)d + (double)val[q]);
    dst[t] = d;
}

// coadd.py:1284-1292 with pad widths (1262-1267): divide the 2f boundary rows/cols by the taper, B, T, L, R
__global__ void trapezoid_recover_kernel(float *__restrict__ maps, long nmaps, int ny, int nx, int fade, int pb, int pt,
                                         int pl, int pr)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= nmaps * ny * nx) return;
    const int x = (int)(t % nx), y = (int)((t / nx) % ny);
    const int fk2 = 2 * fade;
    const double two_pi = 6.283185307179586;
    auto taper = [&](int k) { double s = (double)(k + 1) / (fk2 + 1); return s - sin(two_pi * s) / two_pi; };
    float v = maps[t];
    const int it = ny - pt - 1, ir = nx - pr - 1;
    if (y >= pb && y < pb + fk2) v = (float)((double)v / taper(y - pb));
    if (y <= it && y > it - fk2) v = (float)((double)v / taper(it - y));
    if (x >= pl && x < pl + fk2) v = (float)((double)v / taper(x - pl));
    if (x <= ir && x > ir - fk2) v = (float)((double)v / taper(ir - x));
    maps[t] = v;
}

}  // namespace imcom

using namespace imcom;

extern "C" int imcom_block_accumulate(imcom_ctx *ctx, int batch, const int *jst_host, const int *ist_host, int n2, int fade,
                                      int nlayer, const void *src, int src_is_f64, float *dst, int nside_pf)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && jst_host && ist_host && src && dst && n2 >= 1 && fade >= 0 && nlayer >= 1, "bad arguments");
    const int n2f = n2 + 2 * fade;
    IMCOM_REQUIRE(2 * fade <= n2, "fade=%d: neighbouring stamps must overlap by less than a stamp", fade);
    for (int s = 0; s < batch; s++)
        IMCOM_REQUIRE(jst_host[s] >= 1 && ist_host[s] >= 1 && jst_host[s] * n2 + 2 * fade <= nside_pf && ist_host[s] * n2 + 2 * fade <= nside_pf,
                      "stamp %d (%d,%d) outside the block", s, jst_host[s], ist_host[s]);
    IMCOM_TRY(ws_reserve(ctx, (size_t)batch * 12 + 1024));
    int *jd = (int *)ws_take(ctx, (size_t)batch * 4), *id = (int *)ws_take(ctx, (size_t)batch * 4), *ld = (int *)ws_take(ctx, (size_t)batch * 4);
    // stamps of equal index parity never overlap: four ordered passes make the overlap sums deterministic
    std::vector<int> order;
    int cnt[4] = {0, 0, 0, 0};
    for (int p = 0; p < 4; p++)
        for (int s = 0; s < batch; s++)
            if ((((jst_host[s] & 1) << 1) | (ist_host[s] & 1)) == p) { order.push_back(s); cnt[p]++; }
    // through the pinned ring: the copies read it, not the caller's arrays, so the call returns without draining the stream
    IMCOM_TRY(upload(ctx, jd, jst_host, (size_t)batch));
    IMCOM_TRY(upload(ctx, id, ist_host, (size_t)batch));
    IMCOM_TRY(upload(ctx, ld, order.data(), (size_t)batch));
    ProfScope ps(ctx, "block_acc");
    int off = 0;
    for (int p = 0; p < 4; p++) {
        if (cnt[p] == 0) continue;
        dim3 grid((n2f * n2f + 255) / 256, cnt[p], nlayer);
        if (src_is_f64)
            hipLaunchKernelGGL(block_accumulate_kernel<double>, grid, dim3(256), 0, ctx->stream, cnt[p], ld + off, jd, id, n2, n2f, nlayer,
                               (const double *)src, dst, nside_pf);
        else
            hipLaunchKernelGGL(block_accumulate_kernel<float>, grid, dim3(256), 0, ctx->stream, cnt[p], ld + off, jd, id, n2, n2f, nlayer,
                               (const float *)src, dst, nside_pf);
        off += cnt[p];
    }
    return check_launch("block_accumulate_kernel");
}

extern "C" int imcom_block_place(imcom_ctx *ctx, int batch, const int *jst_host, const int *ist_host, int n2, int fade, int nlayer,
                                 const void *src, int src_is_f64, void *layers, int nside_pf)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && jst_host && ist_host && src && layers && n2 >= 1 && fade >= 0 && nlayer >= 1, "bad arguments");
    const int n2f = n2 + 2 * fade;
    IMCOM_REQUIRE(2 * fade <= n2, "fade=%d: neighbouring stamps must overlap by less than a stamp", fade);
    for (int s = 0; s < batch; s++)
        IMCOM_REQUIRE(jst_host[s] >= 1 && ist_host[s] >= 1 && jst_host[s] * n2 + 2 * fade <= nside_pf && ist_host[s] * n2 + 2 * fade <= nside_pf,
                      "stamp %d (%d,%d) outside the block", s, jst_host[s], ist_host[s]);
    IMCOM_TRY(ws_reserve(ctx, (size_t)batch * 8 + 1024));
    int *jd = (int *)ws_take(ctx, (size_t)batch * 4), *id = (int *)ws_take(ctx, (size_t)batch * 4);
    IMCOM_TRY(upload(ctx, jd, jst_host, (size_t)batch));
    IMCOM_TRY(upload(ctx, id, ist_host, (size_t)batch));
    ProfScope ps(ctx, "block_acc");
    dim3 grid((n2f * n2f + 255) / 256, batch, nlayer);
    if (src_is_f64)
        hipLaunchKernelGGL(block_place_kernel<double>, grid, dim3(256), 0, ctx->stream, batch, jd, id, n2, n2f, nlayer, (const double *)src,
                           (double *)layers, nside_pf);
    else
        hipLaunchKernelGGL(block_place_kernel<float>, grid, dim3(256), 0, ctx->stream, batch, jd, id, n2, n2f, nlayer, (const float *)src,
                           (float *)layers, nside_pf);
    return check_launch("block_place_kernel");
}

extern "C" int imcom_block_combine(imcom_ctx *ctx, int n1P, int n2, int fade, long nlayer, const void *layers, int src_is_f64, float *dst,
                                   int nside_pf, int order, int j_st_min, int i_st_min)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(n1P >= 1 && n1P < 32000 && n2 >= 1 && fade >= 0 && nlayer >= 1 && layers && dst && (order == 0 || order == 1) && j_st_min >= 1 && i_st_min >= 1,
                  "bad arguments");
    const int cells = order, pj = j_st_min & 1, pi = i_st_min & 1;  // (only the parity of the window's origin decides which stamps share a cell)
    IMCOM_REQUIRE(2 * fade <= n2 && nside_pf == n1P * n2 + 2 * fade, "nside_pf = %d is not n1P * n2 + 2 fade (or 2 fade > n2)", nside_pf);
    const long tot = nlayer * nside_pf * nside_pf;
    if (src_is_f64)
        hipLaunchKernelGGL(block_combine_kernel<double>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, n1P, n2, n2 + 2 * fade,
                           nlayer, (const double *)layers, dst, nside_pf, cells, pj, pi);
    else
        hipLaunchKernelGGL(block_combine_kernel<float>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, n1P, n2, n2 + 2 * fade,
                           nlayer, (const float *)layers, dst, nside_pf, cells, pj, pi);
    return check_launch("block_combine_kernel");
}

extern "C" int imcom_trapezoid_recover_f32(imcom_ctx *ctx, float *maps, long nmaps, int ny, int nx, int fade, int pad_b, int pad_t,
                                           int pad_l, int pad_r)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(maps && nmaps >= 0 && ny >= 1 && nx >= 1 && fade >= 0 && pad_b >= 0 && pad_t >= 0 && pad_l >= 0 && pad_r >= 0, "bad arguments");
    if (fade == 0 || nmaps == 0) return IMCOM_OK;
    const long tot = nmaps * ny * nx;
    hipLaunchKernelGGL(trapezoid_recover_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, maps, nmaps, ny, nx, fade,
                       pad_b, pad_t, pad_l, pad_r);
    return check_launch("trapezoid_recover_kernel");
}

// Block.compress_map (reference src/pyimcom/coadd.py:2087-2138): float32 map -> (u)int16 of coef * log10(map),
//   clip(floor(coef * log10(clip(map, 1e-32, None)) + 0.5), a_min, a_max)
// evaluated in float32 as numpy evaluates it for a float32 map (the python scalars are weakly typed); log10 is
// rounded correctly to float32 (computed in double).  NaN inputs map to a_min.
namespace imcom {
__global__ void compress_map_kernel(const float *__restrict__ map, long count, float coef, float a_min, float a_max,
                                    short *__restrict__ out)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float x = fmaxf(map[i], 1e-32f);
    const float l = (float)log10((double)x);
    float v = floorf(__fadd_rn(__fmul_rn(coef, l), 0.5f));
    v = fminf(fmaxf(v, a_min), a_max);
    if (!(v == v)) v = a_min;
    const int iv = (int)v;
    out[i] = (short)(unsigned short)(iv & 0xffff);  // two's complement bits serve both int16 and uint16
}
}  // namespace imcom

extern "C" int imcom_compress_map_f32(imcom_ctx *ctx, const float *map, long count, int coef, int is_unsigned, void *out)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(map && out && count >= 0, "bad arguments");
    if (count == 0) return IMCOM_OK;
    hipLaunchKernelGGL(compress_map_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, map, count, (float)coef,
                       is_unsigned ? 0.0f : -32768.0f, is_unsigned ? 65535.0f : 32767.0f, (short *)out);
    return check_launch("compress_map_kernel");
}

// ---- seam 20: padding stamps shared between neighbouring blocks (reference src/pyimcom/analysis.py:394-537) ----------------------------
// OutImage._update_hdu_data for device-resident blocks: "my" strip towards the neighbour is updated from the neighbour's interior strip.
// padshare_core.h holds the index ranges and the arithmetic; the kernels below only walk the strips.  Each reads the neighbour, reads
// and writes my strip, and touches nothing else.
#include "padshare_core.h"

namespace imcom {

static_assert(PS_NO_FLOOR == IMCOM_PADSHARE_NO_FLOOR, "the floor code that zeroes nothing");

// Strip pixel t of a plane of side n: the position p along the strip axis, and the element offsets in my plane and the neighbour's.
// (A strip has fewer than 2^31 pixels -- the entries check it -- so the one division a pixel is a 32-bit one.)
__device__ __forceinline__ void padshare_pixel(int direction, const PsStrip &s, int n, unsigned t, long my_row, long ur_row, int *p, long *mo, long *uo)
{
    if (ps_along_x(direction)) {
        const unsigned y = t / (unsigned)s.len;
        *p = (int)(t - y * (unsigned)s.len);
        *mo = y * my_row + s.my0 + *p;
        *uo = y * ur_row + s.ur0 + *p;
    } else {
        *p = (int)(t / (unsigned)n);
        const unsigned x = t - (unsigned)*p * (unsigned)n;
        *mo = (s.my0 + *p) * my_row + x;
        *uo = (s.ur0 + *p) * ur_row + x;
    }
}

// 435-450: PRIMARY, plane blockIdx.y
__global__ void padshare_layers_kernel(int direction, int add_mode, int n, int w, int fk, float *__restrict__ mine, long my_row, long my_plane,
                                       const float *__restrict__ theirs, long ur_row, long ur_plane)
{
    const PsStrip s = ps_strip(direction, n, w, fk);
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (unsigned)s.len * (unsigned)n) return;
    int p;
    long mo, uo;
    padshare_pixel(direction, s, n, t, my_row, ur_row, &p, &mo, &uo);
    float *m = mine + blockIdx.y * my_plane + mo;
    *m = ps_combine(*m, theirs[blockIdx.y * ur_plane + uo], add_mode);
}

// 468-486: INWEIGHT [n_out][n_expo][n1P][n1P], pair blockIdx.y of (my_idx, ur_idx); a plain copy
__global__ void padshare_weights_kernel(int direction, int n_out, int n1P, int pad, const int *__restrict__ pairs, float *__restrict__ mine, int n_mine,
                                        const float *__restrict__ theirs, int n_theirs)
{
    const PsStrip s = ps_strip(direction, n1P, pad, 0);
    const unsigned per = (unsigned)s.len * (unsigned)n1P;
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per * (unsigned)n_out) return;
    const unsigned o = t / per;
    int p;
    long mo, uo;
    padshare_pixel(direction, s, n1P, t - o * per, n1P, n1P, &p, &mo, &uo);
    const long plane = (long)n1P * n1P;
    const int my_idx = pairs[2 * blockIdx.y], ur_idx = pairs[2 * blockIdx.y + 1];
    mine[((long)o * n_mine + my_idx) * plane + mo] = theirs[((long)o * n_theirs + ur_idx) * plane + uo];
}

// 498-537: the quality maps, map blockIdx.y / n_out, plane blockIdx.y % n_out: decode both codes, taper both sides in add mode, combine,
// encode, store into my strip
__global__ void padshare_maps_kernel(int direction, int add_mode, int n, int w, int fk, int n_out, const imcom_padshare_map *__restrict__ maps)
{
    const PsStrip s = ps_strip(direction, n, w, fk);
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned per = (unsigned)s.len * (unsigned)n;
    if (t >= per) return;
    const imcom_padshare_map d = maps[blockIdx.y / (unsigned)n_out];
    const unsigned o = blockIdx.y % (unsigned)n_out;
    int p;
    long mo, uo;
    padshare_pixel(direction, s, n, t, n, n, &p, &mo, &uo);
    uint16_t *m = (uint16_t *)d.mine + (long)o * n * n + mo;
    float mv = ps_decode(ps_code(*m, d.is_unsigned), d.decode_coef, d.floor_code);
    float uv = ps_decode(ps_code(((const uint16_t *)d.theirs)[(long)o * n * n + uo], d.is_unsigned), d.decode_coef, d.floor_code);
    if (add_mode) {
        mv = ps_taper(mv, ps_taper_mine(direction, p, w, fk), fk);
        uv = ps_taper(uv, ps_taper_theirs(direction, p, w, fk), fk);
    }
    const float sum = ps_combine(mv, uv, add_mode);
    if (d.sums) d.sums[(long)o * per + t] = sum;
    *m = ps_encode(sum, (float)d.encode_coef, d.is_unsigned);
}

}  // namespace imcom

extern "C" int imcom_padshare_layers(imcom_ctx *ctx, int direction, int add_mode, int nside_p, int width, int fk, long nplanes, float *mine,
                                     long mine_row, long mine_plane, const float *theirs, long theirs_row, long theirs_plane)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(ps_shape_ok(direction, nside_p, width, fk), "direction %d, NsideP %d, width %d, fade kernel %d: not a padding strip (0 <= direction <= 3, "
                  "fk <= width, 2 width <= NsideP)", direction, nside_p, width, fk);
    IMCOM_REQUIRE(mine && theirs && nplanes >= 0 && nplanes <= 65535 && mine_row >= nside_p && theirs_row >= nside_p &&
                  mine_plane >= (nside_p - 1) * mine_row + nside_p && theirs_plane >= (nside_p - 1) * theirs_row + nside_p, "bad arguments");
    IMCOM_REQUIRE(mine != theirs, "a block does not share padding stamps with itself");
    const long tot = (long)(width + fk) * nside_p;
    IMCOM_REQUIRE(tot < (1L << 31), "a strip of %ld pixels", tot);
    if (tot == 0 || nplanes == 0) return IMCOM_OK;
    ProfScope ps(ctx, "padshare");
    hipLaunchKernelGGL(padshare_layers_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)nplanes), dim3(256), 0, ctx->stream, direction, add_mode ? 1 : 0,
                       nside_p, width, fk, mine, mine_row, mine_plane, theirs, theirs_row, theirs_plane);
    return check_launch("padshare_layers_kernel");
}

extern "C" int imcom_padshare_weights(imcom_ctx *ctx, int direction, int n_out, int n1P, int pad, int npairs, const int *pairs_host, float *mine,
                                      int n_mine, const float *theirs, int n_theirs)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(ps_shape_ok(direction, n1P, pad, 0), "direction %d, n1P %d, postage_pad %d: not a padding strip (0 <= direction <= 3, 2 pad <= n1P)",
                  direction, n1P, pad);
    IMCOM_REQUIRE(npairs >= 0 && npairs <= 65535 && n_out >= 0 && n_mine >= 0 && n_theirs >= 0, "bad arguments");
    if (npairs == 0) return IMCOM_OK;
    IMCOM_REQUIRE(pairs_host && mine && theirs, "bad arguments");
    IMCOM_REQUIRE(mine != theirs, "a block does not share padding stamps with itself");
    for (int k = 0; k < npairs; k++) {
        IMCOM_REQUIRE(pairs_host[2 * k] >= 0 && pairs_host[2 * k] < n_mine && pairs_host[2 * k + 1] >= 0 && pairs_host[2 * k + 1] < n_theirs,
                      "pair %d (%d, %d) outside the %d and %d exposures", k, pairs_host[2 * k], pairs_host[2 * k + 1], n_mine, n_theirs);
        for (int j = 0; j < k; j++) IMCOM_REQUIRE(pairs_host[2 * j] != pairs_host[2 * k], "exposure %d of mine is written twice", pairs_host[2 * k]);
    }
    const long tot = (long)pad * n1P * n_out;
    IMCOM_REQUIRE(tot < (1L << 31), "strips of %ld pixels", tot);
    if (tot == 0) return IMCOM_OK;
    IMCOM_TRY(ws_reserve(ctx, (size_t)npairs * 8 + 1024));
    int *pd;
    IMCOM_TRY(ws_take(ctx, (size_t)npairs * 2, &pd, "imcom_padshare_weights"));
    IMCOM_TRY(upload(ctx, pd, pairs_host, (size_t)npairs * 2));
    ProfScope ps(ctx, "padshare");
    hipLaunchKernelGGL(padshare_weights_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)npairs), dim3(256), 0, ctx->stream, direction, n_out, n1P, pad,
                       pd, mine, n_mine, theirs, n_theirs);
    return check_launch("padshare_weights_kernel");
}

extern "C" int imcom_padshare_maps(imcom_ctx *ctx, int direction, int add_mode, int nside_p, int width, int fk, int n_out, int nmaps,
                                   const imcom_padshare_map *maps_host)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(ps_shape_ok(direction, nside_p, width, fk), "direction %d, NsideP %d, width %d, fade kernel %d: not a padding strip (0 <= direction <= 3, "
                  "fk <= width, 2 width <= NsideP)", direction, nside_p, width, fk);
    IMCOM_REQUIRE(nmaps >= 0 && n_out >= 0 && (long)nmaps * n_out <= 65535, "bad arguments");
    const long tot = (long)(width + fk) * nside_p;
    IMCOM_REQUIRE(tot < (1L << 31), "a strip of %ld pixels", tot);
    if (nmaps == 0 || n_out == 0 || tot == 0) return IMCOM_OK;
    IMCOM_REQUIRE(maps_host, "bad arguments");
    for (int k = 0; k < nmaps; k++) {
        const imcom_padshare_map &d = maps_host[k];
        IMCOM_REQUIRE(d.mine && d.theirs && d.decode_coef != 0.0 && d.decode_coef == d.decode_coef && d.encode_coef != 0, "map %d: bad descriptor", k);
        IMCOM_REQUIRE(d.mine != d.theirs, "a block does not share padding stamps with itself");
    }
    IMCOM_TRY(ws_reserve(ctx, (size_t)nmaps * sizeof(imcom_padshare_map) + 1024));
    imcom_padshare_map *md;
    IMCOM_TRY(ws_take(ctx, (size_t)nmaps, &md, "imcom_padshare_maps"));
    IMCOM_TRY(upload(ctx, md, maps_host, (size_t)nmaps));
    ProfScope ps(ctx, "padshare");
    hipLaunchKernelGGL(padshare_maps_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)(nmaps * n_out)), dim3(256), 0, ctx->stream, direction,
                       add_mode ? 1 : 0, nside_p, width, fk, n_out, md);
    return check_launch("padshare_maps_kernel");
}
