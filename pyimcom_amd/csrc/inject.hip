// inject.hip -- injected point-source layers (reference src/pyimcom/layer.py:792-854, GridInject.make_image_from_grid): the PSF of
// every grid star out of a Legendre cube (coadd.py:624-640) and the stars drawn into the SCA image with the D5512 interpolator.
// The C-ABI entries imcom_psf_from_cube / imcom_draw_stars are at the end of the file.
#include "d5512.h"
#include "launchers.h"

namespace imcom {

// out[s][p] = scale * sum_a lpoly[s][a] planes[a][p] (coadd.py:631: einsum("a,aij->ij"), after the smearing -- smooth_and_pad is linear,
// so the na planes are smeared once per call and a star costs this contraction alone).  One thread per pixel and CUBE_STARS stars: a
// plane value is read once for CUBE_STARS outputs, the coefficients are uniform over the workgroup.  The planes (na * npix doubles, well
// under a MiB) stay in L2; the kernel's roof is the HBM write of out.
constexpr int CUBE_STARS = 8;
__global__ __launch_bounds__(256) void cube_contract_kernel(const double *__restrict__ planes, int na, long npix, const double *__restrict__ lpoly,
                                                            int nstar, double scale, double *__restrict__ out)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int s0 = blockIdx.y * CUBE_STARS, ns = min(CUBE_STARS, nstar - s0);
    if (p >= npix) return;
    double acc[CUBE_STARS];
#pragma unroll
    for (int k = 0; k < CUBE_STARS; k++) acc[k] = 0.0;
    for (int a = 0; a < na; a++) {
        const double v = planes[(long)a * npix + p];
#pragma unroll
        for (int k = 0; k < CUBE_STARS; k++)
            if (k < ns) acc[k] += lpoly[(long)(s0 + k) * na + a] * v;
    }
#pragma unroll
    for (int k = 0; k < CUBE_STARS; k++)
        if (k < ns) out[(long)(s0 + k) * npix + p] = scale * acc[k];
}

// ------------------------------------------------------------------------------------------------
// Drawing.  One workgroup owns a DRAW_TILE x DRAW_TILE tile of the image and every pixel of it has one owner thread, which adds the stars
// that reach it in ascending star index -- the reference's loop order (layer.py:825) -- so the image is the same bit for bit from run to
// run and however the star list is cut into calls; there is no atomic.  The workgroup scans the star list 256 stars at a time (one star
// per thread, a 64-bit ballot per wave) and visits the stars whose patch meets the tile.  A star's patch is its clipped box
// (layer.py:827-830) cut down to the native pixels whose sample point lies on the PSF's interpolation grid (routine.py:166-167): about
// (px + 3) / oversamp pixels a side, not 2 d.  The sample points of a star form a separable grid, so its D5512 weights are formed once per
// tile column and per tile row (64 threads) and shared through LDS.
constexpr int DRAW_TILE = 32;
constexpr int DRAW_PAD = 6;  // layer.py:822

// the columns of the image a star may touch along one axis, [lo, hi): the box of layer.py:827-830, cut down (with a margin of a pixel; the
// exact test is made per column) to sample points 4 <= X < ng - 5.  Empty for positions that are not finite or absurd.
__device__ __forceinline__ void star_span(double pos, int n, double oversamp, int d, int nside, int *lo, int *hi)
{
    *lo = 0;
    *hi = 0;
    if (!(pos > -1.0e9 && pos < 1.0e9)) return;
    const int ip = (int)pos;
    const double c = (n - 1) / 2.0 + DRAW_PAD;
    const double a = floor(pos + (4.0 - c) / oversamp) - 1.0, b = ceil(pos + (n + 2 * DRAW_PAD - 5 - c) / oversamp) + 2.0;
    const int l = max(max(0, ip - d), (int)fmax(a, -2.0e9)), h = min(min(nside, ip + d), (int)fmin(b, 2.0e9));
    if (l < h) {
        *lo = l;
        *hi = h;
    }
}

// sample cell and weights of image column (or row) `pix` of a star at `pos`: layer.py:845-846 and routine.py:160-171 in the reference's
// order of operations (no contraction: the cell index is a truncation).  Returns the cell, or -1 when the point is off the grid.
__device__ __forceinline__ int star_cell(int pix, double pos, int n, double oversamp, int lo, int hi, double (&w)[10])
{
    if (pix < lo || pix >= hi) return -1;
    const double X = __dadd_rn(__dadd_rn(__dmul_rn(oversamp, (double)pix - pos), (n - 1) / 2.0), (double)DRAW_PAD);
    const int xi = to_cell(X);
    if (xi < 4 || xi >= n + 2 * DRAW_PAD - 5) return -1;
    d5512_getw(w, X - xi - 0.5);
    return xi;
}

__global__ __launch_bounds__(256) void draw_stars_kernel(int nstar, const double *__restrict__ psfs, int py, int px, const double *__restrict__ xsca,
                                                         const double *__restrict__ ysca, double oversamp, double oversamp2, int d, int nside,
                                                         double *__restrict__ image)
{
    __shared__ unsigned long long smask[4];
    __shared__ double wgt[2][10][DRAW_TILE];  // [x, y][tap][column / row of the tile]
    __shared__ int cell[2][DRAW_TILE];
    const int t = threadIdx.x, tx = t & (DRAW_TILE - 1), tr = t / DRAW_TILE;  // rows tr + 8 k
    const int x0 = blockIdx.x * DRAW_TILE, y0 = blockIdx.y * DRAW_TILE;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    bool touched[4] = {false, false, false, false};

    for (int base = 0; base < nstar; base += 256) {
        const int s = base + t;
        bool hit = false;
        if (s < nstar) {
            int lo, hi;
            star_span(xsca[s], px, oversamp, d, nside, &lo, &hi);
            hit = lo < x0 + DRAW_TILE && hi > x0;
            if (hit) {
                star_span(ysca[s], py, oversamp, d, nside, &lo, &hi);
                hit = lo < y0 + DRAW_TILE && hi > y0;
            }
        }
        const unsigned long long m = __ballot(hit);
        if ((t & 63) == 0) smask[t >> 6] = m;
        __syncthreads();
        unsigned long long mw[4] = {smask[0], smask[1], smask[2], smask[3]};
        __syncthreads();
        for (int w = 0; w < 4; w++) {
            while (mw[w]) {  // ascending star index
                const int star = base + w * 64 + __ffsll((long long)mw[w]) - 1;
                mw[w] &= mw[w] - 1;
                if (t < 2 * DRAW_TILE) {
                    const int axis = t / DRAW_TILE, l = t & (DRAW_TILE - 1);
                    const double pos = axis ? ysca[star] : xsca[star];
                    const int n = axis ? py : px;
                    int lo, hi;
                    star_span(pos, n, oversamp, d, nside, &lo, &hi);
                    double wv[10];
                    const int c = star_cell((axis ? y0 : x0) + l, pos, n, oversamp, lo, hi, wv);
                    cell[axis][l] = c;
                    if (c >= 0) {
#pragma unroll
                        for (int k = 0; k < 10; k++) wgt[axis][k][l] = wv[k];
                    }
                }
                __syncthreads();
                const int xi = cell[0][tx];
                if (xi >= 0) {
                    double wx[10];
#pragma unroll
                    for (int j = 0; j < 10; j++) wx[j] = wgt[0][j][tx];
                    const double *P = psfs + (long)star * py * px;
                    const int cx0 = xi - 4 - DRAW_PAD;  // first tap in the unpadded image
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int r = tr + 8 * k, yi = cell[1][r];
                        if (yi < 0) continue;
                        const int cy0 = yi - 4 - DRAW_PAD;
                        double out = 0.0;  // x taps inside, y taps outside (routine.py:176-180); taps in the zero padding add nothing
                        for (int i = 0; i < 10; i++) {
                            const int ry = cy0 + i;
                            if (ry < 0 || ry >= py) continue;
                            const double *row = P + (long)ry * px;
                            double strip = 0.0;
#pragma unroll
                            for (int j = 0; j < 10; j++) {
                                const int cx = cx0 + j;
                                if (cx >= 0 && cx < px) strip += wx[j] * row[cx];
                            }
                            out += strip * wgt[1][i][r];
                        }
                        if (!touched[k]) {
                            acc[k] = image[(long)(y0 + r) * nside + (x0 + tx)];
                            touched[k] = true;
                        }
                        acc[k] = __dadd_rn(acc[k], __dmul_rn(out, oversamp2));  // layer.py:849-852
                    }
                }
                __syncthreads();
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (touched[k]) image[(long)(y0 + tr + 8 * k) * nside + (x0 + tx)] = acc[k];  // (touched: the pixel is inside the image, star_span)
}

static int launch_cube_contract(imcom_ctx *ctx, const double *planes, int na, long npix, const double *lpoly, int nstar, double scale, double *out)
{
    if (nstar == 0) return IMCOM_OK;
    ProfScope ps(ctx, "inject_psf");
    hipLaunchKernelGGL(cube_contract_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)((nstar + CUBE_STARS - 1) / CUBE_STARS)), dim3(256), 0,
                       ctx->stream, planes, na, npix, lpoly, nstar, scale, out);
    return check_launch("cube_contract_kernel");
}

static int launch_draw_stars(imcom_ctx *ctx, int nstar, const double *psfs, int py, int px, const double *xsca, const double *ysca, double oversamp,
                      int d, int nside, double *image)
{
    if (nstar == 0) return IMCOM_OK;
    ProfScope ps(ctx, "inject_draw");
    const unsigned nt = (unsigned)((nside + DRAW_TILE - 1) / DRAW_TILE);
    hipLaunchKernelGGL(draw_stars_kernel, dim3(nt, nt), dim3(256), 0, ctx->stream, nstar, psfs, py, px, xsca, ysca, oversamp, oversamp * oversamp, d,
                       nside, image);
    return check_launch("draw_stars_kernel");
}

}  // namespace imcom

using namespace imcom;

// ---------------------------------------------------------------------------------------------
// C entries: injected star layers

extern "C" {

int imcom_psf_from_cube(imcom_ctx *ctx, int na, const double *cube, int ny, int nx, int nstar, const double *lpoly, double tophatwidth,
                        double gaussiansigma, double scale, double *out, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(na >= 1 && cube && ny >= 1 && nx >= 1 && nstar >= 0 && (nstar == 0 || (lpoly && out)), "bad arguments");
    IMCOM_REQUIRE(tophatwidth >= 0.0 && gaussiansigma >= 0.0 && tophatwidth + 6.0 * gaussiansigma < 4096.0 && scale == scale,
                  "bad smearing widths or scale");
    if (nstar == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    const int npad = imcom_smooth_pad_width(tophatwidth, gaussiansigma), nyy = ny + 2 * npad, nxx = nx + 2 * npad;
    const size_t szCube = (size_t)na * ny * nx, szL = (size_t)nstar * na, npix = (size_t)nyy * nxx, szOut = (size_t)nstar * npix;
    WsPlan plan;
    plan.add(smooth_pad_ws_bytes(na, ny, nx, tophatwidth, gaussiansigma));
    plan.add((size_t)na * npix * 8);
    st.plan(plan, {szCube * 8, szL * 8, szOut * 8});
    IMCOM_TRY(ws_reserve(ctx, plan.total));
    SmoothPadWs w;
    IMCOM_TRY(smooth_pad_take(ctx, na, ny, nx, tophatwidth, gaussiansigma, &w, __func__));
    double *planes, *out_d;
    IMCOM_TRY(ws_take(ctx, (size_t)na * npix, &planes, __func__));
    const double *cube_d, *lpoly_d;
    IMCOM_TRY(st.in(cube, szCube, &cube_d));
    IMCOM_TRY(st.in(lpoly, szL, &lpoly_d));
    IMCOM_TRY(st.out(out, szOut, &out_d));
    IMCOM_TRY(smooth_pad_device(ctx, w, na, cube_d, ny, nx, tophatwidth, gaussiansigma, planes));
    IMCOM_TRY(launch_cube_contract(ctx, planes, na, (long)npix, lpoly_d, nstar, scale, out_d));
    IMCOM_TRY(st.back(out, out_d, szOut));
    return st.done();
}

int imcom_draw_stars(imcom_ctx *ctx, int nstar, const double *psfs, int py, int px, const double *xsca, const double *ysca, double oversamp,
                     int d, int nside, double *image, int memspace)
{
    IMCOM_TRY(enter(ctx));
    IMCOM_REQUIRE(nstar >= 0 && image && (nstar == 0 || (psfs && xsca && ysca)), "null pointer");
    IMCOM_REQUIRE(py >= 1 && px >= 1 && py <= 16384 && px <= 16384 && d >= 1 && d <= 65536 && nside >= 1 && nside <= 65536, "bad sizes");
    IMCOM_REQUIRE(oversamp >= 1.0e-3 && oversamp <= 1.0e6, "oversamp %g out of range", oversamp);
    if (nstar == 0) return IMCOM_OK;
    Stage st(ctx, memspace, __func__);
    const size_t szP = (size_t)nstar * py * px, szI = (size_t)nside * nside;
    WsPlan plan;
    st.plan(plan, {szP * 8, (size_t)nstar * 8, (size_t)nstar * 8, szI * 8});
    if (st.host) IMCOM_TRY(ws_reserve(ctx, plan.total));
    const double *p_d, *x_d, *y_d;
    double *img_d;
    IMCOM_TRY(st.in(psfs, szP, &p_d));
    IMCOM_TRY(st.in(xsca, (size_t)nstar, &x_d));
    IMCOM_TRY(st.in(ysca, (size_t)nstar, &y_d));
    IMCOM_TRY(st.inout(image, szI, &img_d));  // the stars are added to what the image holds
    IMCOM_TRY(launch_draw_stars(ctx, nstar, p_d, py, px, x_d, y_d, oversamp, d, nside, img_d));
    IMCOM_TRY(st.back(image, img_d, szI));
    return st.done();
}

}  // extern "C"
