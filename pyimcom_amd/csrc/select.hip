// select.hip -- input-pixel selection of an output stamp on the device.
//
// Replaces OutStamp._process_input_stamps (reference src/pyimcom/coadd.py:886-977) with
// InStamp.make_selection (716-749): the nine InStamps around an output stamp contribute, in order, the pixels
// with (x - x_pivot)^2 + (y - y_pivot)^2 < radius^2 (a missing pivot coordinate drops its term; no pivot at all
// takes every pixel), concatenated into x / y / indata / exposure index and the ten running counts
// (inpix_cumsum).  Pure index work apart from the distance test, which is evaluated exactly as numpy does
// (square, add, compare; no fused multiply-add), so the selection is bit-identical.
#include "common.h"

namespace imcom {

__global__ __launch_bounds__(256) void select_pixels_kernel(const double *__restrict__ pool_x, const double *__restrict__ pool_y,
                                                            const float *__restrict__ pool_data, long npool, int n_inframe,
                                                            const int *__restrict__ pool_expo, const long *__restrict__ inst_off,
                                                            const int *__restrict__ inst_id, const double *__restrict__ pivot_x,
                                                            const double *__restrict__ pivot_y, double radius, int ldn,
                                                            double *__restrict__ x, double *__restrict__ y,
                                                            float *__restrict__ indata, int *__restrict__ expo,
                                                            int *__restrict__ cumsum, int *__restrict__ status)
{
    __shared__ int wcnt[4], total;
    const int s = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double r2 = __dmul_rn(radius, radius);
    if (threadIdx.x == 0) { total = 0; cumsum[s * 10] = 0; }
    __syncthreads();
    for (int idx = 0; idx < 9; idx++) {
        const int inst = inst_id[s * 9 + idx];
        if (inst >= 0) {
            const long o0 = inst_off[inst], o1 = inst_off[inst + 1];
            const double px = pivot_x[s * 9 + idx], py = pivot_y[s * 9 + idx];
            const bool all = (isnan(px) && isnan(py)) || isnan(radius);
            for (long c0 = o0; c0 < o1; c0 += 256) {
                const long i = c0 + threadIdx.x;
                bool in = false;
                double xi = 0.0, yi = 0.0;
                if (i < o1) {
                    xi = pool_x[i];
                    yi = pool_y[i];
                    double d = 0.0;
                    if (!isnan(px)) { const double dx = __dsub_rn(xi, px); d = __dadd_rn(d, __dmul_rn(dx, dx)); }
                    if (!isnan(py)) { const double dy = __dsub_rn(yi, py); d = __dadd_rn(d, __dmul_rn(dy, dy)); }
                    in = all || d < r2;
                }
                const unsigned long long mask = __ballot(in);
                if (lane == 0) wcnt[wave] = __popcll(mask);
                __syncthreads();
                int off = total;
                for (int w = 0; w < wave; w++) off += wcnt[w];
                off += __popcll(mask & ((1ull << lane) - 1ull));
                if (in && off < ldn) {
                    const long o = (long)s * ldn + off;
                    x[o] = xi;
                    y[o] = yi;
                    expo[o] = pool_expo[i];
                    for (int f = 0; f < n_inframe; f++) indata[((long)s * n_inframe + f) * ldn + off] = pool_data[f * npool + i];
                }
                __syncthreads();
                if (threadIdx.x == 0) total += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
                __syncthreads();
            }
        }
        if (threadIdx.x == 0) cumsum[s * 10 + idx + 1] = total;
    }
    __syncthreads();
    const int n = total;
    if (n > ldn) {
        if (threadIdx.x == 0) atomicMax(status, n);
        return;
    }
    for (int i = n + threadIdx.x; i < ldn; i += 256) {  // padding: zeros
        const long o = (long)s * ldn + i;
        x[o] = 0.0;
        y[o] = 0.0;
        expo[o] = 0;
        for (int f = 0; f < n_inframe; f++) indata[((long)s * n_inframe + f) * ldn + i] = 0.0f;
    }
}

}  // namespace imcom

using namespace imcom;

extern "C" int imcom_select_pixels(imcom_ctx *ctx, int batch, const double *pool_x, const double *pool_y, const float *pool_data,
                                   long npool, int n_inframe, const int *pool_expo, const long *inst_off, int n_inst,
                                   const int *inst_id, const double *pivot_x, const double *pivot_y, double radius, int ldn,
                                   double *x, double *y, float *indata, int *expo, int *cumsum, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(batch >= 1 && npool >= 0 && n_inframe >= 1 && n_inst >= 1 && ldn >= 1, "bad sizes");
    IMCOM_REQUIRE(inst_off && inst_id && pivot_x && pivot_y && x && y && indata && expo && cumsum, "null pointer");
    IMCOM_REQUIRE(npool == 0 || (pool_x && pool_y && pool_data && pool_expo), "null pool pointer");
    Stage st(ctx, memspace, __func__);
    const size_t nb = (size_t)batch, np = (size_t)npool, nd = nb * ldn;
    WsPlan plan;
    st.plan(plan, {np * 8, np * 8, np * 4 * n_inframe, np * 4, (size_t)(n_inst + 1) * 8, nb * 9 * 4, nb * 9 * 8, nb * 9 * 8,  // inputs
                   nd * 8, nd * 8, nd * 4 * n_inframe, nd * 4, nb * 40});                                                  // outputs
    plan.add(65536);
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *px_, *py_, *vx_, *vy_;
    const float *pd_;
    const int *pe_, *ii_;
    const long *io_;
    IMCOM_TRY(st.in(pool_x, np, &px_));
    IMCOM_TRY(st.in(pool_y, np, &py_));
    IMCOM_TRY(st.in(pool_data, np * n_inframe, &pd_));
    IMCOM_TRY(st.in(pool_expo, np, &pe_));
    IMCOM_TRY(st.in(inst_off, (size_t)(n_inst + 1), &io_));
    IMCOM_TRY(st.in(inst_id, nb * 9, &ii_));
    IMCOM_TRY(st.in(pivot_x, nb * 9, &vx_));
    IMCOM_TRY(st.in(pivot_y, nb * 9, &vy_));
    double *x_d, *y_d;
    float *d_d;
    int *e_d, *c_d, *status;
    IMCOM_TRY(st.out(x, nd, &x_d));
    IMCOM_TRY(st.out(y, nd, &y_d));
    IMCOM_TRY(st.out(indata, nd * n_inframe, &d_d));
    IMCOM_TRY(st.out(expo, nd, &e_d));
    IMCOM_TRY(st.out(cumsum, nb * 10, &c_d));
    IMCOM_TRY(ws_take(ctx, 1, &status, __func__));
    IMCOM_HIP_CHECK(hipMemsetAsync(status, 0, 4, ctx->stream));
    { ProfScope ps(ctx, "select");
    hipLaunchKernelGGL(select_pixels_kernel, dim3(batch), dim3(256), 0, ctx->stream, px_, py_, pd_, npool, n_inframe, pe_, io_, ii_, vx_, vy_, radius,
                       ldn, x_d, y_d, d_d, e_d, c_d, status); }
    IMCOM_TRY(check_launch("select_pixels_kernel"));
    int sel = 0;
    IMCOM_HIP_CHECK(hipMemcpyAsync(&sel, status, 4, hipMemcpyDeviceToHost, ctx->stream));
    IMCOM_TRY(st.back(x, x_d, nd));
    IMCOM_TRY(st.back(y, y_d, nd));
    IMCOM_TRY(st.back(indata, d_d, nd * n_inframe));
    IMCOM_TRY(st.back(expo, e_d, nd));
    IMCOM_TRY(st.back(cumsum, c_d, nb * 10));
    IMCOM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // in either memory space: the status word is read here
    IMCOM_REQUIRE(sel == 0, "a stamp selects %d input pixels, more than ldn=%d", sel, ldn);
    return IMCOM_OK;
}
