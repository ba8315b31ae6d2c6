// partition.hip -- input pixels of one image binned into postage stamps on the device.
//
// Replaces the binning loop of InImage.partition_pixels (reference src/pyimcom/coadd.py:329-358): pixels are
// visited in a fixed order (sparse-grid cell by cell, row-major inside a cell), dropped when outside
// (pix_lower, pix_upper), masked, or in a stamp the block does not use, and appended to their stamp
// (j_st, i_st) = floor((pos - pix_lower) / n2).  The order inside every stamp is the visiting order, so this is a
// STABLE partition by stamp: a stable least-significant-digit radix sort of (stamp key, visit index) pairs (own kernels
// below: 6-bit digits, two passes for up to 4095 stamps), segment starts from the sorted keys, then a gather.  The WCS
// evaluation that produces the positions stays on the host for imcom_partition_pixels; imcom_partition_wcs (the end of the file) forms the
// positions from two WCS descriptors where they are used, and imcom_extract_layers / imcom_pool_assemble carry the result into the pool that
// the Block seam reads.
#include <vector>

#include "launchers.h"
#include "layers_core.h"
#include "partition_core.h"
#include "wcs_core.h"

namespace imcom {

// ---- stable LSD radix sort of 32-bit keys with their 32-bit payloads, 6 bits per pass --------------------------------
// A workgroup of 256 threads owns RS_TILE consecutive elements; wave w the RS_TILE / 4 consecutive ones from w * RS_TILE / 4,
// lane-consecutive in every step of 64, so "earlier in the array" = (earlier wave, earlier step, lower lane).
constexpr int RS_BITS = 6, RS_BINS = 1 << RS_BITS, RS_STEPS = 8, RS_TILE = 4 * 64 * RS_STEPS;

// hist[d * nblk + b] = number of elements of workgroup b with digit d (digit-major: one exclusive scan over the whole array
// then gives every (digit, workgroup) its first output position)
__global__ __launch_bounds__(256) void radix_hist_kernel(const unsigned int *__restrict__ keys, long n, int shift, int nblk,
                                                         unsigned int *__restrict__ hist)
{
    __shared__ unsigned int h[RS_BINS];
    if (threadIdx.x < RS_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * RS_TILE;
    for (int q = threadIdx.x; q < RS_TILE; q += 256) {
        const long p = base + q;
        if (p < n) atomicAdd(&h[(keys[p] >> shift) & (RS_BINS - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < RS_BINS) hist[(long)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of `count` values in place, one workgroup (the array has 64 x nblk entries: a few hundred thousand)
__global__ __launch_bounds__(1024) void radix_scan_kernel(unsigned int *__restrict__ a, long count)
{
    __shared__ unsigned int part[1024];
    const int t = threadIdx.x;
    const long per = (count + 1023) / 1024, lo = (long)t * per, hi = lo + per < count ? lo + per : count;
    unsigned int sum = 0;
    for (long i = lo; i < hi; i++) sum += a[i];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned int v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned int run = part[t] - sum;  // exclusive prefix of this thread's range
    for (long i = lo; i < hi; i++) { const unsigned int v = a[i]; a[i] = run; run += v; }
}

// vals_in == nullptr: the payload is the element's index (first pass)
__global__ __launch_bounds__(256) void radix_scatter_kernel(const unsigned int *__restrict__ keys_in, const unsigned int *__restrict__ vals_in,
                                                            long n, int shift, int nblk, const unsigned int *__restrict__ base,
                                                            unsigned int *__restrict__ keys_out, unsigned int *__restrict__ vals_out)
{
    __shared__ unsigned int cnt[4][RS_BINS];  // running count per wave and digit, then the wave's exclusive offset
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cnt[tid >> 6][tid & 63] = 0;
    __syncthreads();
    const long p0 = (long)blockIdx.x * RS_TILE + (long)wave * (RS_TILE / 4);
    const unsigned long long lt = (1ULL << lane) - 1;
    unsigned int key[RS_STEPS], rank[RS_STEPS];
#pragma unroll
    for (int s = 0; s < RS_STEPS; s++) {
        const long p = p0 + s * 64 + lane;
        const bool on = p < n;
        key[s] = on ? keys_in[p] : 0xffffffffu;
        const unsigned int d = (key[s] >> shift) & (RS_BINS - 1);
        unsigned long long peers = __ballot(on);  // lanes that carry an element with my digit
#pragma unroll
        for (int b = 0; b < RS_BITS; b++) {
            const unsigned long long bal = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bal : ~bal;
        }
        rank[s] = cnt[wave][d] + __popcll(peers & lt);
        __builtin_amdgcn_wave_barrier();  // every lane has read the running count before the leader advances it
        if (on && (peers & lt) == 0) cnt[wave][d] += __popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (tid < RS_BINS) {  // totals of the four waves -> exclusive offsets among them
        unsigned int run = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const unsigned int c = cnt[w][tid]; cnt[w][tid] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RS_STEPS; s++) {
        const long p = p0 + s * 64 + lane;
        if (p < n) {
            const unsigned int d = (key[s] >> shift) & (RS_BINS - 1);
            const unsigned int o = base[(long)d * nblk + blockIdx.x] + cnt[wave][d] + rank[s];
            keys_out[o] = key[s];
            vals_out[o] = vals_in ? vals_in[p] : (unsigned int)p;
        }
    }
}

// sorts (k0, index) by the low `bits` bits of the keys; the result is in (*ko, *vo), which point into the buffers given
static int radix_sort_pairs(imcom_ctx *ctx, unsigned int *k0, unsigned int *k1, unsigned int *v0, unsigned int *v1, long n, int bits,
                            unsigned int *hist, unsigned int **ko, unsigned int **vo)
{
    const int nblk = (int)((n + RS_TILE - 1) / RS_TILE);
    unsigned int *kin = k0, *kout = k1, *vin = nullptr, *vout = v0;
    for (int shift = 0; shift < bits; shift += RS_BITS) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(256), 0, ctx->stream, kin, n, shift, nblk, hist);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, hist, (long)RS_BINS * nblk);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(256), 0, ctx->stream, kin, vin, n, shift, nblk, hist, kout, vout);
        IMCOM_TRY(check_launch("radix sort pass"));
        unsigned int *t = kin; kin = kout; kout = t;
        vin = vout;
        vout = vout == v0 ? v1 : v0;
    }
    *ko = kin;
    *vo = vin;
    return IMCOM_OK;
}

// Python's float floor division a // b for b > 0 (numpy npy_divmod): exact remainder first
__device__ inline double py_floordiv(double a, double b)
{
    const double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && mod < 0.0) div -= 1.0;
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
}

// The stamp key of a pixel at (x, y) of the block (coadd.py:343-351): nst * nst (dropped: sorts behind every stamp) outside (lo, hi) -- NaN
// fails the strict comparisons --, masked, or in a stamp the block does not use.
__device__ inline unsigned int partition_key(double x, double y, bool unmasked, const unsigned char *__restrict__ use, int nst, double n2, double lo,
                                             double hi)
{
    unsigned int key = (unsigned int)(nst * nst);
    if (lo < x && x < hi && lo < y && y < hi && unmasked) {
        const int ist = (int)py_floordiv(x - lo, n2), jst = (int)py_floordiv(y - lo, n2);
        if (ist >= 0 && ist < nst && jst >= 0 && jst < nst && use[jst * nst + ist]) key = (unsigned int)(jst * nst + ist);
    }
    return key;
}

__global__ void partition_key_kernel(const double *__restrict__ ox, const double *__restrict__ oy,
                                     const unsigned char *__restrict__ mask, const unsigned char *__restrict__ use, int nst,
                                     double n2, double lo, double hi, long npix, unsigned int *__restrict__ keys)
{
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    keys[p] = partition_key(ox[p], oy[p], !mask || mask[p], use, nst, n2, lo, hi);
}

// start[k] = first sorted position of key k (npix where absent); one thread per sorted position
__global__ void partition_bounds_kernel(const unsigned int *__restrict__ keys, long npix, int nkeys, unsigned int *__restrict__ start)
{
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned int k = keys[p];
    if (p == 0 || keys[p - 1] != k) {
        if (k <= (unsigned int)nkeys) start[k] = (unsigned int)p;
    }
}

__global__ void partition_count_kernel(const unsigned int *__restrict__ start, int nkeys, long npix, unsigned int *__restrict__ count,
                                       int npixmax, int *__restrict__ status)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nkeys) return;
    unsigned int s = start[k], e = (unsigned int)npix;
    if (s == 0xffffffffu) { count[k] = 0; return; }
    for (int q = k + 1; q <= nkeys; q++)
        if (start[q] != 0xffffffffu) { e = start[q]; break; }
    count[k] = e - s;
    if ((long)(e - s) > npixmax) atomicMax(status, (int)(e - s));
}

__global__ void partition_gather_kernel(const unsigned int *__restrict__ keys, const unsigned int *__restrict__ vals,
                                        const unsigned int *__restrict__ start, long npix, int nkeys, int npixmax,
                                        const double *__restrict__ ox, const double *__restrict__ oy,
                                        const unsigned short *__restrict__ ix, const unsigned short *__restrict__ iy,
                                        unsigned short *__restrict__ y_idx, unsigned short *__restrict__ x_idx,
                                        double *__restrict__ y_val, double *__restrict__ x_val)
{
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned int k = keys[p];
    if (k >= (unsigned int)nkeys) return;
    const long slot = p - start[k];
    if (slot >= npixmax) return;
    const unsigned int v = vals[p];
    const long o = (long)k * npixmax + slot;
    y_idx[o] = iy[v];
    x_idx[o] = ix[v];
    y_val[o] = oy[v];
    x_val[o] = ox[v];
}


// ---- the same partition with the positions formed from two WCSs (imcom_partition_wcs) -------------------------------------------------------
// A visit index is decoded to its pixel by partition_core.h and the pixel's position in the block is wcs_core.h's wcs_pix2pix, origin 0, with
// the NaN rule of wcs_pix2pix_kernel (wcs.hip): the same arithmetic on the same integer pixel, so the same bits as imcom_wcs_pix2pix returns.
// The position is formed twice -- for the key of every visited pixel, and again for the pixels that are kept, where it is stored -- instead of
// being parked in 16 bytes a visited pixel in between.
struct PartWcs {
    WcsDesc from, to;
    WcsTab tf, tt;
    double M[9];
};

struct PartVisit {
    const unsigned int *start, *cell;  // partition_cells' lists
    const unsigned short *sp_arr;
    int ncell, sp_res;
};

__device__ __forceinline__ void partition_wcs_position(const PartWcs &w, int x, int y, double *xo, double *yo)
{
    double xf, yf;
    if (!wcs_pix2pix(w.from, w.tf, w.to, w.tt, w.M, (double)x, (double)y, 0, &xf, &yf) || !(xf - xf == 0.0 && yf - yf == 0.0)) xf = NAN, yf = NAN;
    *xo = xf, *yo = yf;
}

// mask: the frame mask [nside][nside] (null: none)
__global__ __launch_bounds__(256) void partition_wcs_key_kernel(const PartWcs w, const PartVisit v, const unsigned char *__restrict__ mask, int nside,
                                                                const unsigned char *__restrict__ use, int nst, double n2, double lo, double hi, long npix,
                                                                unsigned int *__restrict__ keys)
{
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    int x, y;
    partition_decode(v.start, v.cell, v.ncell, v.sp_arr, v.sp_res, (unsigned int)p, &y, &x);
    double xf, yf;
    partition_wcs_position(w, x, y, &xf, &yf);
    keys[p] = partition_key(xf, yf, !mask || mask[(long)y * nside + x], use, nst, n2, lo, hi);
}

__global__ __launch_bounds__(256) void partition_wcs_gather_kernel(const PartWcs w, const PartVisit vis, const unsigned int *__restrict__ keys,
                                                                   const unsigned int *__restrict__ vals, const unsigned int *__restrict__ start, long npix,
                                                                   int nkeys, int npixmax, unsigned short *__restrict__ y_idx, unsigned short *__restrict__ x_idx,
                                                                   double *__restrict__ y_val, double *__restrict__ x_val)
{
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned int k = keys[p];
    if (k >= (unsigned int)nkeys) return;
    const long slot = p - start[k];
    if (slot >= npixmax) return;
    int x, y;
    partition_decode(vis.start, vis.cell, vis.ncell, vis.sp_arr, vis.sp_res, vals[p], &y, &x);
    double xf, yf;
    partition_wcs_position(w, x, y, &xf, &yf);
    const long o = (long)k * npixmax + slot;
    y_idx[o] = (unsigned short)y;
    x_idx[o] = (unsigned short)x;
    y_val[o] = yf;
    x_val[o] = xf;
}

// InImage.extract_layers (coadd.py:394-404): data[f][s][k] = indata[f][y_idx[s][k]][x_idx[s][k]] for k < pix_count[s], zero beyond; one thread
// per element of data [n_inframe][nstamps][max_count].
__global__ __launch_bounds__(256) void extract_layers_kernel(const float *__restrict__ indata, int n_inframe, int nside, const unsigned short *__restrict__ y_idx,
                                                             const unsigned short *__restrict__ x_idx, const unsigned int *__restrict__ count, int nstamps,
                                                             int npixmax, int max_count, float *__restrict__ data)
{
    const long per = (long)nstamps * max_count, q = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (q >= per) return;
    const int s = (int)(q / max_count), k = (int)(q - (long)s * max_count);
    const bool on = k < npixmax && (unsigned int)k < count[s];
    long at = 0;
    if (on) {
        const int y = y_idx[(long)s * npixmax + k], x = x_idx[(long)s * npixmax + k];
        at = y < nside && x < nside ? (long)y * nside + x : -1;
    }
    for (int f = 0; f < n_inframe; f++) data[f * per + q] = on && at >= 0 ? indata[(long)f * nside * nside + at] : 0.0f;
}

// InStamp.__init__ (coadd.py:688-707) for every stamp of a block: workgroup (s, m) copies the count[m][s] pixels of image m in stamp s from
// the image's lists (at src_xy / src_d elements from their starts) to dst[m][s] of the pool.  One owner per pool element; no sort.
struct PoolTables {
    const unsigned long long *xp, *yp, *dp;  // [n_img] device addresses: x, y float64, data float32 [n_inframe] frame_stride apart
    const long *frame_stride;                // [n_img]
    const unsigned int *count;               // [n_img][nstamps]
    const long *src_xy, *src_d, *dst;        // [n_img][nstamps]
    const int *expo_of;                      // [n_img]
};

__global__ __launch_bounds__(128) void pool_assemble_kernel(const PoolTables t, int nstamps, int n_inframe, long npool, double *__restrict__ x,
                                                            double *__restrict__ y, float *__restrict__ data, int *__restrict__ expo)
{
    const int s = blockIdx.x, m = blockIdx.y;
    const long e = (long)m * nstamps + s;
    const unsigned int n = t.count[e];
    if (n == 0) return;
    const double *sx = (const double *)t.xp[m] + t.src_xy[e], *sy = (const double *)t.yp[m] + t.src_xy[e];
    const float *sd = (const float *)t.dp[m] + t.src_d[e];
    const long fs = t.frame_stride[m], d0 = t.dst[e];
    const int ex = t.expo_of[m];
    for (unsigned int k = threadIdx.x; k < n; k += blockDim.x) {
        x[d0 + k] = sx[k];
        y[d0 + k] = sy[k];
        if (expo) expo[d0 + k] = ex;
        for (int f = 0; f < n_inframe; f++) data[f * npool + d0 + k] = sd[f * fs + k];
    }
}

}  // namespace imcom

using namespace imcom;

extern "C" int imcom_partition_pixels(imcom_ctx *ctx, long npix, const double *out_x, const double *out_y, const unsigned short *in_x,
                                      const unsigned short *in_y, const unsigned char *mask, const unsigned char *use_instamps, int nst,
                                      int n2, double pix_lower, double pix_upper, int npixmax, unsigned short *y_idx,
                                      unsigned short *x_idx, double *y_val, double *x_val, unsigned int *pix_count)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(npix >= 0 && npix < (1L << 32) - 2 && nst >= 1 && n2 >= 1 && npixmax >= 1, "bad sizes");
    IMCOM_REQUIRE(use_instamps && y_idx && x_idx && y_val && x_val && pix_count, "null pointer");
    IMCOM_REQUIRE(npix == 0 || (out_x && out_y && in_x && in_y), "null input pointer");
    const int nkeys = nst * nst;
    hipStream_t st = ctx->stream;
    int bits = 1;
    while ((1L << bits) <= nkeys) bits++;  // keys 0 .. nkeys (nkeys = dropped)
    const long nblk = (npix + RS_TILE - 1) / RS_TILE;
    IMCOM_TRY(ws_reserve(ctx, (size_t)npix * 16 + (size_t)nblk * RS_BINS * 4 + (size_t)(nkeys + 2) * 4 + 8192));
    unsigned int *k0 = (unsigned int *)ws_take(ctx, (size_t)npix * 4 + 4), *k1 = (unsigned int *)ws_take(ctx, (size_t)npix * 4 + 4);
    unsigned int *v0 = (unsigned int *)ws_take(ctx, (size_t)npix * 4 + 4), *v1 = (unsigned int *)ws_take(ctx, (size_t)npix * 4 + 4);
    unsigned int *hist = (unsigned int *)ws_take(ctx, (size_t)nblk * RS_BINS * 4 + 16);
    unsigned int *start = (unsigned int *)ws_take(ctx, (size_t)(nkeys + 1) * 4);
    int *status = (int *)ws_take(ctx, 4);
    if (!k0 || !k1 || !v0 || !v1 || !hist || !start || !status) return ws_short(__func__);
    unsigned int *ks = k0, *vs = v0;  // the sorted pairs
    IMCOM_HIP_CHECK(hipMemsetAsync(start, 0xff, (size_t)(nkeys + 1) * 4, st));
    IMCOM_HIP_CHECK(hipMemsetAsync(status, 0, 4, st));
    if (npix > 0) {
        const unsigned nb = (unsigned)((npix + 255) / 256);
        hipLaunchKernelGGL(partition_key_kernel, dim3(nb), dim3(256), 0, st, out_x, out_y, mask, use_instamps, nst, (double)n2, pix_lower,
                           pix_upper, npix, k0);
        IMCOM_TRY(check_launch("partition_key_kernel"));
        IMCOM_TRY(radix_sort_pairs(ctx, k0, k1, v0, v1, npix, bits, hist, &ks, &vs));
        hipLaunchKernelGGL(partition_bounds_kernel, dim3(nb), dim3(256), 0, st, ks, npix, nkeys, start);
    }
    hipLaunchKernelGGL(partition_count_kernel, dim3((nkeys + 255) / 256), dim3(256), 0, st, start, nkeys, npix, pix_count, npixmax, status);
    if (npix > 0) {
        const unsigned nb = (unsigned)((npix + 255) / 256);
        hipLaunchKernelGGL(partition_gather_kernel, dim3(nb), dim3(256), 0, st, ks, vs, start, npix, nkeys, npixmax, out_x, out_y, in_x, in_y,
                           y_idx, x_idx, y_val, x_val);
    }
    IMCOM_TRY(check_launch("partition kernels"));
    int sth = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(&sth, status, 4, hipMemcpyDeviceToHost, st));
    IMCOM_HIP_CHECK(hipStreamSynchronize(st));
    IMCOM_REQUIRE(sth == 0, "a stamp receives %d pixels of this image, more than npixmax=%d (coadd.py:270-279)", sth, npixmax);
    return IMCOM_OK;
}

extern "C" int imcom_partition_wcs(imcom_ctx *ctx, const double *from, const void *ftab, int ftab_f64, int ftab_n2, double ftab_lo, double ftab_hi, const double *to,
                                   const void *ttab, int ttab_f64, int ttab_n2, double ttab_lo, double ttab_hi, const unsigned short *sp_arr,
                                   const unsigned char *relevant, int sp_res, int nside, const unsigned char *mask, const unsigned char *use_instamps, int nst, int n2,
                                   double pix_lower, double pix_upper, int npixmax, unsigned short *y_idx, unsigned short *x_idx, double *y_val, double *x_val,
                                   unsigned int *pix_count, long *nvisited)
{
    const char *who = "partition_wcs";
    IMCOM_TRY(enter(ctx));
    PartWcs w;
    IMCOM_TRY(wcs_descriptor(from, who, &w.from));
    IMCOM_TRY(wcs_descriptor(to, who, &w.to));
    IMCOM_TRY(wcs_table_check(ftab, ftab_f64, ftab_n2, ftab_lo, ftab_hi, who));
    IMCOM_TRY(wcs_table_check(ttab, ttab_f64, ttab_n2, ttab_lo, ttab_hi, who));
    w.tf = ftab ? WcsTab{ftab, ftab_f64 ? 1 : 0, ftab_n2, ftab_lo, ftab_hi} : WcsTab{nullptr, 0, 0, 0.0, 0.0};
    w.tt = ttab ? WcsTab{ttab, ttab_f64 ? 1 : 0, ttab_n2, ttab_lo, ttab_hi} : WcsTab{nullptr, 0, 0, 0.0, 0.0};
    wcs_rotation_product(w.from, w.to, w.M);
    IMCOM_REQUIRE(sp_res >= 1 && sp_res <= 4096 && nside >= 1 && nside <= 65535 && nst >= 1 && nst <= 2048 && n2 >= 1 && npixmax >= 1, "%s: bad sizes", who);
    IMCOM_REQUIRE(sp_arr && relevant && use_instamps && y_idx && x_idx && y_val && x_val && pix_count, "%s: null pointer", who);
    for (int k = 0; k < sp_res; k++) IMCOM_REQUIRE(sp_arr[k] <= sp_arr[k + 1], "%s: sp_arr decreases at node %d", who, k + 1);
    IMCOM_REQUIRE(sp_arr[sp_res] <= nside, "%s: sp_arr ends at %d, beyond the frame of %d pixels a side", who, (int)sp_arr[sp_res], nside);
    std::vector<unsigned int> cstart((size_t)sp_res * sp_res + 1), cell((size_t)sp_res * sp_res);
    const int ncell = partition_cells(sp_arr, relevant, sp_res, cstart.data(), cell.data());
    const long npix = (long)cstart[ncell];
    if (nvisited) *nvisited = npix;
    const int nkeys = nst * nst;
    hipStream_t st = ctx->stream;
    int bits = 1;
    while ((1L << bits) <= nkeys) bits++;  // keys 0 .. nkeys (nkeys = dropped)
    const long nblk = (npix + RS_TILE - 1) / RS_TILE;
    WsPlan plan;
    for (int k = 0; k < 4; k++) plan.add((size_t)npix * 4 + 4);
    plan.add((size_t)nblk * RS_BINS * 4 + 16);
    plan.add((size_t)(nkeys + 1) * 4);
    plan.add(4);
    plan.add((size_t)(ncell + 1) * 4);
    plan.add((size_t)(ncell + 1) * 4);
    plan.add((size_t)(sp_res + 1) * 2);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned int *k0, *k1, *v0, *v1, *hist, *start, *cstart_d, *cell_d;
    int *status;
    unsigned short *sp_d;
    IMCOM_TRY(ws_take(ctx, (size_t)npix + 1, &k0, who));
    IMCOM_TRY(ws_take(ctx, (size_t)npix + 1, &k1, who));
    IMCOM_TRY(ws_take(ctx, (size_t)npix + 1, &v0, who));
    IMCOM_TRY(ws_take(ctx, (size_t)npix + 1, &v1, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nblk * RS_BINS + 4, &hist, who));
    IMCOM_TRY(ws_take(ctx, (size_t)nkeys + 1, &start, who));
    IMCOM_TRY(ws_take(ctx, 1, &status, who));
    IMCOM_TRY(ws_take(ctx, (size_t)ncell + 1, &cstart_d, who));
    IMCOM_TRY(ws_take(ctx, (size_t)ncell + 1, &cell_d, who));
    IMCOM_TRY(ws_take(ctx, (size_t)sp_res + 1, &sp_d, who));
    IMCOM_TRY(upload(ctx, cstart_d, cstart.data(), (size_t)ncell + 1));
    IMCOM_TRY(upload(ctx, cell_d, cell.data(), (size_t)ncell));
    IMCOM_TRY(upload(ctx, sp_d, sp_arr, (size_t)sp_res + 1));
    const PartVisit vis = {cstart_d, cell_d, sp_d, ncell, sp_res};
    unsigned int *ks = k0, *vs = v0;  // the sorted pairs
    IMCOM_HIP_CHECK(hipMemsetAsync(start, 0xff, (size_t)(nkeys + 1) * 4, st));
    IMCOM_HIP_CHECK(hipMemsetAsync(status, 0, 4, st));
    const unsigned nb = (unsigned)((npix + 255) / 256);
    if (npix > 0) {
        hipLaunchKernelGGL(partition_wcs_key_kernel, dim3(nb), dim3(256), 0, st, w, vis, mask, nside, use_instamps, nst, (double)n2, pix_lower, pix_upper, npix, k0);
        IMCOM_TRY(check_launch("partition_wcs_key_kernel"));
        IMCOM_TRY(radix_sort_pairs(ctx, k0, k1, v0, v1, npix, bits, hist, &ks, &vs));
        hipLaunchKernelGGL(partition_bounds_kernel, dim3(nb), dim3(256), 0, st, ks, npix, nkeys, start);
    }
    hipLaunchKernelGGL(partition_count_kernel, dim3((nkeys + 255) / 256), dim3(256), 0, st, start, nkeys, npix, pix_count, npixmax, status);
    if (npix > 0)
        hipLaunchKernelGGL(partition_wcs_gather_kernel, dim3(nb), dim3(256), 0, st, w, vis, ks, vs, start, npix, nkeys, npixmax, y_idx, x_idx, y_val, x_val);
    IMCOM_TRY(check_launch("partition_wcs kernels"));
    int sth = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(&sth, status, 4, hipMemcpyDeviceToHost, st));
    IMCOM_HIP_CHECK(hipStreamSynchronize(st));
    IMCOM_REQUIRE(sth == 0, "a stamp receives %d pixels of this image, more than npixmax=%d (coadd.py:270-279)", sth, npixmax);
    return IMCOM_OK;
}

extern "C" int imcom_extract_layers(imcom_ctx *ctx, const float *indata, int n_inframe, int nside, const unsigned short *y_idx, const unsigned short *x_idx,
                                    const unsigned int *pix_count, int nstamps, int npixmax, int max_count, float *data)
{
    const char *who = "extract_layers";
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(n_inframe >= 1 && nside >= 1 && nside <= 65535 && nstamps >= 1 && npixmax >= 1 && max_count >= 0, "%s: bad sizes", who);
    const long per = (long)nstamps * max_count;
    if (per == 0) return IMCOM_OK;
    IMCOM_REQUIRE(indata && y_idx && x_idx && pix_count && data, "%s: null pointer", who);
    hipLaunchKernelGGL(extract_layers_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, ctx->stream, indata, n_inframe, nside, y_idx, x_idx, pix_count, nstamps,
                       npixmax, max_count, data);
    return check_launch("extract_layers_kernel");
}

// The cube that imcom_extract_layers reads, plane by plane (kernel and launcher: layers.hip).
extern "C" int imcom_layer_place(imcom_ctx *ctx, const void *src, int src_type, int src_swapped, int src_ny, int src_nx, int y0, int x0, int flip, int op,
                                 double sub, int post_scale_flag, double scale, float *dst, int nside, int memspace)
{
    const char *who = "layer_place";
    IMCOM_TRY(enter(ctx));
    static const char *const rule[] = {"", "the source type is 0 .. 5 (float32, float64, int16, uint16, int32, uint8)", "src_swapped and post_scale_flag are 0 or 1",
                                       "flip is 0 (none), 1 (x) or 2 (y)", "op is 0 (none) or 1 (subtract)", "sides are 0 .. 65536",
                                       "the window leaves the source"};
    const int broken = layer_place_check(src_type, src_swapped, src_ny, src_nx, y0, x0, flip, op, post_scale_flag, nside);
    IMCOM_REQUIRE(broken == 0, "%s: %s (type %d, source %d x %d, origin (%d, %d), flip %d, op %d, nside %d)", who, rule[broken], src_type, src_ny, src_nx, y0, x0, flip,
                  op, nside);
    IMCOM_REQUIRE(memspace == IMCOM_MEM_HOST || memspace == IMCOM_MEM_DEVICE, "%s: memspace %d", who, memspace);
    if (nside == 0) return IMCOM_OK;
    IMCOM_REQUIRE(src && dst, "%s: null pointer", who);
    const size_t esz = (size_t)layer_type_size(src_type), nsrc = (size_t)src_ny * src_nx, ndst = (size_t)nside * nside;
    IMCOM_REQUIRE(memspace == IMCOM_MEM_HOST || ((uintptr_t)src % esz == 0 && (uintptr_t)dst % 4 == 0), "%s: a pointer is not aligned to its element", who);
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    st.plan(plan, {nsrc * esz, ndst * 4});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const char *s_d;
    float *d_d;
    IMCOM_TRY(st.in((const char *)src, nsrc * esz, &s_d));
    IMCOM_TRY(st.out(dst, ndst, &d_d));
    IMCOM_TRY(launch_layer_place(ctx, s_d, src_type, src_swapped, src_nx, y0, x0, flip, op, sub, post_scale_flag, scale, d_d, nside));
    IMCOM_TRY(st.back(dst, (const float *)d_d, ndst));
    return st.done();
}

extern "C" int imcom_pool_assemble(imcom_ctx *ctx, int n_img, int nstamps, int n_inframe, const void *const *x_src, const void *const *y_src,
                                   const void *const *data_src, const long *xy_pitch, const long *data_pitch, const long *frame_stride, const int *expo_of,
                                   const unsigned int *count, long npool, double *x, double *y, float *data, int *expo, long *inst_off)
{
    const char *who = "pool_assemble";
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(n_img >= 0 && n_img <= 65535 && nstamps >= 1 && n_inframe >= 1 && npool >= 0, "%s: bad sizes", who);
    IMCOM_REQUIRE(inst_off && (n_img == 0 || (x_src && y_src && data_src && xy_pitch && data_pitch && frame_stride && expo_of && count)), "%s: null pointer", who);
    const size_t ne = (size_t)n_img * nstamps;
    // the prefix sums: a stamp's pixels are the images' in list order (coadd.py:698-707), the stamps row-major
    std::vector<long> off((size_t)nstamps + 1, 0), dst(ne), sxy(ne), sd(ne);
    for (int s = 0; s < nstamps; s++) {
        long run = off[s];
        for (int m = 0; m < n_img; m++) {
            dst[(size_t)m * nstamps + s] = run;
            run += count[(size_t)m * nstamps + s];
        }
        off[s + 1] = run;
    }
    IMCOM_REQUIRE(off[nstamps] == npool, "%s: the counts sum to %ld pixels, the pool holds %ld", who, off[nstamps], npool);
    std::vector<unsigned long long> ptrs((size_t)3 * n_img);
    for (int m = 0; m < n_img; m++) {
        IMCOM_REQUIRE(xy_pitch[m] >= 0 && data_pitch[m] >= 0 && frame_stride[m] >= 0, "%s: image %d has a negative pitch", who, m);
        long run = 0;  // pitch 0: the image's lists are compact, stamp after stamp
        bool any = false;
        for (int s = 0; s < nstamps; s++) {
            const size_t e = (size_t)m * nstamps + s;
            IMCOM_REQUIRE((xy_pitch[m] == 0 || count[e] <= (unsigned long)xy_pitch[m]) && (data_pitch[m] == 0 || count[e] <= (unsigned long)data_pitch[m]),
                          "%s: image %d has %u pixels in stamp %d, more than its pitch", who, m, count[e], s);
            sxy[e] = xy_pitch[m] ? s * xy_pitch[m] : run;
            sd[e] = data_pitch[m] ? s * data_pitch[m] : run;
            run += count[e];
            any = any || count[e];
        }
        IMCOM_REQUIRE(!any || (x_src[m] && y_src[m] && data_src[m]), "%s: image %d has pixels and a null list", who, m);
        ptrs[m] = (unsigned long long)(uintptr_t)x_src[m];
        ptrs[(size_t)n_img + m] = (unsigned long long)(uintptr_t)y_src[m];
        ptrs[(size_t)2 * n_img + m] = (unsigned long long)(uintptr_t)data_src[m];
    }
    IMCOM_TRY(upload(ctx, inst_off, off.data(), (size_t)nstamps + 1));
    if (npool == 0 || n_img == 0) return IMCOM_OK;
    IMCOM_REQUIRE(x && y && data, "%s: null pointer", who);  // (expo may be null: an image's own lists carry none)
    WsPlan plan;
    plan.add((size_t)3 * n_img * 8);
    plan.add((size_t)n_img * 8);
    plan.add((size_t)n_img * 4);
    plan.add(ne * 4);
    for (int k = 0; k < 3; k++) plan.add(ne * 8);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    unsigned long long *ptrs_d;
    long *fs_d, *sxy_d, *sd_d, *dst_d;
    int *ex_d;
    unsigned int *cnt_d;
    IMCOM_TRY(ws_take(ctx, (size_t)3 * n_img, &ptrs_d, who));
    IMCOM_TRY(ws_take(ctx, (size_t)n_img, &fs_d, who));
    IMCOM_TRY(ws_take(ctx, (size_t)n_img, &ex_d, who));
    IMCOM_TRY(ws_take(ctx, ne, &cnt_d, who));
    IMCOM_TRY(ws_take(ctx, ne, &sxy_d, who));
    IMCOM_TRY(ws_take(ctx, ne, &sd_d, who));
    IMCOM_TRY(ws_take(ctx, ne, &dst_d, who));
    IMCOM_TRY(upload(ctx, ptrs_d, ptrs.data(), (size_t)3 * n_img));
    IMCOM_TRY(upload(ctx, fs_d, frame_stride, (size_t)n_img));
    IMCOM_TRY(upload(ctx, ex_d, expo_of, (size_t)n_img));
    IMCOM_TRY(upload(ctx, cnt_d, count, ne));
    IMCOM_TRY(upload(ctx, sxy_d, sxy.data(), ne));
    IMCOM_TRY(upload(ctx, sd_d, sd.data(), ne));
    IMCOM_TRY(upload(ctx, dst_d, dst.data(), ne));
    const PoolTables t = {ptrs_d, ptrs_d + n_img, ptrs_d + 2 * (size_t)n_img, fs_d, cnt_d, sxy_d, sd_d, dst_d, ex_d};
    hipLaunchKernelGGL(pool_assemble_kernel, dim3((unsigned)nstamps, (unsigned)n_img), dim3(128), 0, ctx->stream, t, nstamps, n_inframe, npool, x, y, data, expo);
    return check_launch("pool_assemble_kernel");
}
