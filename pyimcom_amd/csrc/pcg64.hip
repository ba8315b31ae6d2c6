// pcg64.hip -- counter-based draws of numpy's PCG64 stream and the simulated cosmic-ray mask built from them (reference
// src/pyimcom/layer.py:933-964, Mask.randmask; 1071-1077, the lab-noise threshold of Mask.load_cr_mask; 313-401, GalSimInject.subgen /
// subgen_multirow).  The C-ABI entries imcom_pcg64_uniform / imcom_pcg64_uniform_at / imcom_cr_mask are at the end of the file.
//
// PCG64 (XSL-RR 128/64) is the 128-bit LCG s <- PCG64_MULT s + inc (mod 2^128) with the output rotr64(hi ^ lo, s >> 122), taken AFTER the
// step.  Draw k (from 0) of Generator.random() / uniform() is (out_k >> 11) 2^-53 with out_k the output of the state after k + 1 steps.
// The d-step map is affine, s -> A s + C, and the maps of 2^j steps (PCG64_JUMPS pairs, formed on the host for this inc) compose to any d:
// one 128-bit multiply-add per set bit of d.  Everything is integer arithmetic until the one exact conversion, so every result has one
// right value and no result depends on how the work is cut into threads, blocks or calls.
#include "launchers.h"
#include "pcg64_dev.h"

namespace imcom {

// one step; the double of the new state
__device__ __forceinline__ double draw(U128 &s, const U128 *tab)
{
    s = affine(tab[0], s, tab[1]);
    const unsigned long long x = s.hi ^ s.lo;
    const unsigned rot = (unsigned)(s.hi >> 58);
    const unsigned long long out = (x >> rot) | (x << ((64u - rot) & 63u));  // (rot = 0: both shifts are by 0)
    return (double)(out >> 11) * 0x1.0p-53;
}

// out[i] = U[offset + i]: a thread forms PCG64_RUN consecutive draws, one jump and then steps
constexpr int PCG64_RUN = 8;
__global__ __launch_bounds__(256) void pcg64_uniform_kernel(U128 state, const unsigned long long *__restrict__ jumps, U128 offset, long count,
                                                            double *__restrict__ out)
{
    __shared__ U128 tab[2 * PCG64_JUMPS];
    load_jumps(tab, jumps);
    __syncthreads();
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * PCG64_RUN;
    if (i0 >= count) return;
    const unsigned long long dlo = offset.lo + (unsigned long long)i0;
    U128 s = jump(state, dlo, offset.hi + (dlo < offset.lo), tab);
    const int n = (int)min((long)PCG64_RUN, count - i0);
    for (int q = 0; q < n; q++) out[i0 + q] = draw(s, tab);
}

// out[i] = U[pos[i]], pos in any order (a negative entry counts as its value mod 2^64)
__global__ __launch_bounds__(256) void pcg64_uniform_at_kernel(U128 state, const unsigned long long *__restrict__ jumps, const long *__restrict__ pos,
                                                               long count, double *__restrict__ out)
{
    __shared__ U128 tab[2 * PCG64_JUMPS];
    load_jumps(tab, jumps);
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    U128 s = jump(state, (unsigned long long)pos[i], 0ull, tab);
    out[i] = draw(s, tab);
}

// ------------------------------------------------------------------------------------------------
// Mask.randmask.  Pixel (r, c) of the padded W x W slice (W = nside + 2 pad) is draw slice W^2 + r W + c; it is a hit when that draw is
// below pcut, and output pixel (y, x) is good when none of the nine padded pixels around (y + pad, x + pad) is a hit (the 3 x 3 convolution
// of layer.py:963; its zero border is never reached because pad >= 1).  A workgroup owns CR_TX x CR_TY output pixels.  Their hits are the
// 64 x 32 padded pixels from (y0 + pad - 1, x0 + pad - 1): thread t forms the 8 of row t / 8 from column 8 (t % 8), as one byte of that
// row's 64-bit word in LDS -- the only form the draws ever take in memory.  Three row words OR-ed and smeared by two bits then answer a row
// of outputs.  Padded rows and columns beyond pad + nside are not formed.
constexpr int CR_TX = 62, CR_TY = 30;
__global__ __launch_bounds__(256) void cr_mask_kernel(U128 state, const unsigned long long *__restrict__ jumps, unsigned long long base, int nside, int pad,
                                                      double pcut, const float *__restrict__ labnoise, double threshold, unsigned char *__restrict__ mask,
                                                      unsigned long long *__restrict__ ngood)
{
    __shared__ U128 tab[2 * PCG64_JUMPS];
    __shared__ unsigned long long rows[CR_TY + 2];
    __shared__ unsigned int good_lds;
    const int t = threadIdx.x, x0 = blockIdx.x * CR_TX, y0 = blockIdx.y * CR_TY;
    load_jumps(tab, jumps);
    if (t == 0) good_lds = 0;
    __syncthreads();
    {
        const int hr = t >> 3, seg = t & 7;
        const int r = y0 + pad - 1 + hr, c0 = x0 + pad - 1 + 8 * seg, last = pad + nside;  // last padded row / column that is looked at
        unsigned bits = 0;
        if (r <= last && c0 <= last) {
            const unsigned long long W = (unsigned long long)nside + 2ull * pad;
            U128 s = jump(state, base + (unsigned long long)r * W + (unsigned long long)c0, 0ull, tab);
            const int n = min(8, last - c0 + 1);
            for (int q = 0; q < n; q++) bits |= (draw(s, tab) < pcut ? 1u : 0u) << q;
        }
        ((unsigned char *)rows)[8 * hr + seg] = (unsigned char)bits;  // little endian: bit c of rows[hr] is column c of the window
    }
    __syncthreads();
    unsigned good = 0;
    for (int o = t; o < CR_TX * CR_TY; o += 256) {
        const int ly = o / CR_TX, lx = o - ly * CR_TX, y = y0 + ly, x = x0 + lx;
        if (y >= nside || x >= nside) continue;
        const unsigned long long m = rows[ly] | rows[ly + 1] | rows[ly + 2];
        bool ok = (((m | (m >> 1) | (m >> 2)) >> lx) & 1ull) == 0ull;
        if (labnoise) ok = ok && (double)fabsf(labnoise[(long)y * nside + x]) < threshold;  // (a NaN compares false, as numpy's does)
        mask[(long)y * nside + x] = ok ? 1 : 0;
        good += ok ? 1u : 0u;
    }
    atomicAdd(&good_lds, good);
    __syncthreads();
    if (t == 0 && good_lds) atomicAdd(ngood, (unsigned long long)good_lds);  // (integer: the same total in any order)
}

static int launch_pcg64_uniform(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const unsigned long long offset[2], long count,
                         double *out)
{
    if (count == 0) return IMCOM_OK;
    ProfScope ps(ctx, "pcg64_uniform");
    const long per_block = 256L * PCG64_RUN;
    hipLaunchKernelGGL(pcg64_uniform_kernel, dim3((unsigned)((count + per_block - 1) / per_block)), dim3(256), 0, ctx->stream, U128{state[0], state[1]}, jumps,
                       U128{offset[0], offset[1]}, count, out);
    return check_launch("pcg64_uniform_kernel");
}

static int launch_pcg64_uniform_at(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, const long *pos, long count, double *out)
{
    if (count == 0) return IMCOM_OK;
    ProfScope ps(ctx, "pcg64_uniform");
    hipLaunchKernelGGL(pcg64_uniform_at_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, U128{state[0], state[1]}, jumps, pos, count,
                       out);
    return check_launch("pcg64_uniform_at_kernel");
}

static int launch_cr_mask(imcom_ctx *ctx, const unsigned long long state[2], const unsigned long long *jumps, unsigned long long base, int nside, int pad, double pcut,
                   const float *labnoise, double threshold, unsigned char *mask, unsigned long long *ngood)
{
    ProfScope ps(ctx, "cr_mask");
    IMCOM_HIP_CHECK(hipMemsetAsync(ngood, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(cr_mask_kernel, dim3((unsigned)((nside + CR_TX - 1) / CR_TX), (unsigned)((nside + CR_TY - 1) / CR_TY)), dim3(256), 0, ctx->stream,
                       U128{state[0], state[1]}, jumps, base, nside, pad, pcut, labnoise, threshold, mask, ngood);
    return check_launch("cr_mask_kernel");
}

// the affine maps of 2^j steps of s <- M s + inc, j < PCG64_JUMPS, into the workspace: (A_0, C_0) = (M, inc), A_{j+1} = A_j^2,
// C_{j+1} = (A_j + 1) C_j (mod 2^128)
int pcg64_jumps(imcom_ctx *ctx, uint64_t inc_lo, uint64_t inc_hi, const unsigned long long **jumps_d, const char *who)
{
    typedef unsigned __int128 u128;
    unsigned long long tab[PCG64_JUMPS * 4], *d;
    u128 A = ((u128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull, Cc = ((u128)inc_hi << 64) | inc_lo;
    for (int j = 0; j < PCG64_JUMPS; j++) {
        tab[4 * j] = (unsigned long long)A;
        tab[4 * j + 1] = (unsigned long long)(A >> 64);
        tab[4 * j + 2] = (unsigned long long)Cc;
        tab[4 * j + 3] = (unsigned long long)(Cc >> 64);
        Cc = (A + 1) * Cc;
        A = A * A;
    }
    IMCOM_TRY(ws_take(ctx, (size_t)PCG64_JUMPS * 4, &d, who));
    IMCOM_TRY(upload(ctx, d, tab, (size_t)PCG64_JUMPS * 4));
    *jumps_d = d;
    return IMCOM_OK;
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: PCG64 draws by position and the cosmic-ray mask

extern "C" {

int imcom_pcg64_uniform(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, uint64_t offset_lo, uint64_t offset_hi,
                        long count, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    IMCOM_REQUIRE(count == 0 || out, "null pointer");
    if (count == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {(size_t)count * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi}, offset[2] = {offset_lo, offset_hi};
    double *o_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.out(out, (size_t)count, &o_d));
    IMCOM_TRY(launch_pcg64_uniform(ctx, state, jumps, offset, count, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)count));
    return st.done();
}

int imcom_pcg64_uniform_at(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, const long *pos, long count, double *out,
                           int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(count >= 0 && count <= PCG64_MAX_COUNT, "pcg64: count %ld outside 0 .. 2^36", count);
    IMCOM_REQUIRE(count == 0 || (pos && out), "null pointer");
    if (count == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {(size_t)count * 8, (size_t)count * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi};
    const long *p_d;
    double *o_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.in(pos, (size_t)count, &p_d));
    IMCOM_TRY(st.out(out, (size_t)count, &o_d));
    IMCOM_TRY(launch_pcg64_uniform_at(ctx, state, jumps, p_d, count, o_d));
    IMCOM_TRY(st.back(out, (const double *)o_d, (size_t)count));
    return st.done();
}

int imcom_cr_mask(imcom_ctx *ctx, uint64_t state_lo, uint64_t state_hi, uint64_t inc_lo, uint64_t inc_hi, int nside, int pad, int slice, int n_slices,
                  double pcut, const float *labnoise, double threshold, unsigned char *mask, long *ngood, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(mask && ngood, "null pointer");
    IMCOM_REQUIRE(nside >= 1 && nside <= 65536 && pad >= 1 && pad <= 4096, "cr_mask: nside %d outside 1 .. 65536 or pad %d outside 1 .. 4096", nside, pad);
    IMCOM_REQUIRE(n_slices >= 1 && n_slices <= 65536 && slice >= 0 && slice < n_slices, "cr_mask: slice %d of %d", slice, n_slices);
    Stage st(ctx, memspace, __func__);
    const size_t npix = (size_t)nside * nside;
    const unsigned long long W = (unsigned long long)nside + 2ull * pad;  // (slice W^2 + W^2 < 2^16 2^34)
    WsPlan plan;
    plan.add((size_t)PCG64_JUMPS * 32);
    st.plan(plan, {labnoise ? npix * 4 : 0, npix, sizeof(long)});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const unsigned long long *jumps, state[2] = {state_lo, state_hi};
    const float *l_d;
    unsigned char *m_d;
    long *n_d;
    IMCOM_TRY(pcg64_jumps(ctx, inc_lo, inc_hi, &jumps, __func__));
    IMCOM_TRY(st.in(labnoise, npix, &l_d));
    IMCOM_TRY(st.out(mask, npix, &m_d));
    IMCOM_TRY(st.out(ngood, (size_t)1, &n_d));
    IMCOM_TRY(launch_cr_mask(ctx, state, jumps, (unsigned long long)slice * W * W, nside, pad, pcut, l_d, threshold, m_d, (unsigned long long *)n_d));
    IMCOM_TRY(st.back(mask, (const unsigned char *)m_d, npix));
    IMCOM_TRY(st.back(ngood, (const long *)n_d, (size_t)1));
    return st.done();
}

}  // extern "C"
