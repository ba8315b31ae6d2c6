// mosaic_check.cpp -- csrc/mosaic_core.h as a host program (built with -fsanitize=address,undefined by tests/test_metamosaic_host.py).
// Reads a file of 64-bit words: the number of jobs, then per job
//   0, symin, symax, sxmin, sxmax, cy, cx, by, bx, ns                       a window: the index maps and the row split against plain loops
//   1, ns, n, n x (x, y, r as the bits of doubles), ceil(ns ns / 8) words   circles and the expected mask, eight pixels a word
//   2, type, divisor (0: -0.1, 1: 0.1), bits of bels, n, n x (code, bits of the expected float32)
// Prints "<what> <checked> <failures>" for windows, splits, caps, pixels and decibels; exit status 1 on any failure.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mosaic_core.h"

using namespace imcom;

static std::vector<int64_t> words;
static size_t at = 0;
static int64_t next() { return words.at(at++); }
static double next_double()
{
    const int64_t w = next();
    double d;
    memcpy(&d, &w, 8);
    return d;
}

static long n_windows = 0, bad_windows = 0, n_splits = 0, bad_splits = 0, n_caps = 0, bad_caps = 0, n_pixels = 0, bad_pixels = 0, n_db = 0, bad_db = 0;

// One row of w elements moved as mosaic_paste_kernel moves it, on element indices: every destination element exactly once, 16-byte pieces
// aligned on both sides.
template <typename T>
static void split_row(uint64_t dst_addr, uint64_t src_addr, int w, std::vector<int> &times)
{
    int lead, nvec;
    mo_row_split(dst_addr, src_addr, w, (int)sizeof(T), &lead, &nvec);
    const int per = 16 / (int)sizeof(T);
    n_splits++;
    if (lead < 0 || lead > w || nvec < 0 || lead + nvec * per > w) {
        bad_splits++;
        return;
    }
    for (int k = 0; k < nvec; k++) {
        const uint64_t d = dst_addr + (uint64_t)(lead + k * per) * sizeof(T), s = src_addr + (uint64_t)(lead + k * per) * sizeof(T);
        if (d % 16 || s % 16) bad_splits++;
        for (int j = 0; j < per; j++) times.at(lead + k * per + j)++;
    }
    const int tail = lead + nvec * per;
    for (int k = 0; k < lead + (w - tail); k++) times.at(k < lead ? k : tail + (k - lead))++;
    // where both sides agree in their offset within 16 bytes, all but fewer than two pieces' worth of elements go in pieces
    if ((dst_addr & 15) == (src_addr & 15) && w - nvec * per >= 2 * per) bad_splits++;
}

static void window_job()
{
    MoWindow W;
    W.symin = (int)next(); W.symax = (int)next(); W.sxmin = (int)next(); W.sxmax = (int)next(); W.cy = (int)next(); W.cx = (int)next();
    const int by = (int)next(), bx = (int)next(), ns = (int)next();
    n_windows++;
    if (!mo_window_ok(W, by, bx, ns)) {
        bad_windows++;
        return;
    }
    // plain loops: mosaic[y + cy][x + cx] = file[y][x]
    std::vector<long> want((size_t)ns * ns, -1), got((size_t)ns * ns, -1);
    for (int y = W.symin; y < W.symax; y++)
        for (int x = W.sxmin; x < W.sxmax; x++) want.at((size_t)(y + W.cy) * ns + (x + W.cx)) = (long)y * bx + x;
    for (int r = 0; r < mo_rows(W); r++) {
        const long s0 = mo_src_offset(W, r, bx), d0 = mo_dst_offset(W, r, ns);
        for (int c = 0; c < mo_cols(W); c++) got.at((size_t)(d0 + c)) = s0 + c;
        for (int es = 4; es <= 8; es += 4)
            for (uint64_t dm = 0; dm < 16; dm += es)
                for (uint64_t sm = 0; sm < 16; sm += es) {
                    std::vector<int> times((size_t)mo_cols(W), 0);
                    const uint64_t da = 4096 + dm + (uint64_t)d0 * es, sa = 8192 + sm + (uint64_t)s0 * es;
                    if (es == 4) split_row<uint32_t>(da, sa, mo_cols(W), times);
                    else split_row<uint64_t>(da, sa, mo_cols(W), times);
                    for (int t : times)
                        if (t != 1) bad_splits++;
                }
    }
    if (want != got) bad_windows++;
}

static void caps_job()
{
    const int ns = (int)next();
    const long n = next();
    std::vector<double> x(n), y(n), r(n);
    for (long i = 0; i < n; i++) { x[i] = next_double(); y[i] = next_double(); r[i] = next_double(); }
    std::vector<unsigned char> want((size_t)ns * ns);
    for (size_t k = 0; k < want.size(); k += 8) {
        const uint64_t w = (uint64_t)next();
        for (size_t j = 0; j < 8 && k + j < want.size(); j++) want[k + j] = (w >> (8 * j)) & 0xff;
    }
    n_caps++;
    // the kernel's form: boxes, their prefix sum, one flat index space
    std::vector<MoBox> box(n);
    std::vector<long> start(n + 1, 0);
    for (long i = 0; i < n; i++) {
        box[i] = mo_cap_box(x[i], y[i], r[i], ns);
        if (box[i].x0 < 0 || box[i].y0 < 0 || box[i].w < 0 || box[i].h < 0 || box[i].x0 + box[i].w > ns || box[i].y0 + box[i].h > ns) bad_caps++;
        start[i + 1] = start[i] + mo_box_pixels(box[i]);
    }
    std::vector<unsigned char> flat((size_t)ns * ns, 0), plain((size_t)ns * ns, 0);
    long obj = 0;
    for (long p = 0; p < start[n]; p++) {
        while (p >= start[obj + 1]) obj++;
        int ix, iy;
        mo_box_pixel(box[obj], p - start[obj], &ix, &iy);
        n_pixels++;
        if (ix < box[obj].x0 || ix >= box[obj].x0 + box[obj].w || iy < box[obj].y0 || iy >= box[obj].y0 + box[obj].h ||
            (long)(iy - box[obj].y0) * box[obj].w + (ix - box[obj].x0) != p - start[obj]) {
            bad_pixels++;
            continue;
        }
        if (mo_cap_hit(ix, iy, x[obj], y[obj], r[obj])) flat.at((size_t)iy * ns + ix) = 1;
    }
    // lines 341-352 as plain loops, with the reference's own clamps (max with 0 below, min with ns above)
    for (long i = 0; i < n; i++) {
        const double lo_x = std::floor(x[i] - r[i]), hi_x = std::ceil(x[i] + r[i]) + 1, lo_y = std::floor(y[i] - r[i]), hi_y = std::ceil(y[i] + r[i]) + 1;
        const long xmin = lo_x > 0 ? (lo_x > 1e9 ? (long)1e9 : (long)lo_x) : 0, xmax = hi_x < ns ? (hi_x < -1e9 ? (long)-1e9 : (long)hi_x) : ns;
        const long ymin = lo_y > 0 ? (lo_y > 1e9 ? (long)1e9 : (long)lo_y) : 0, ymax = hi_y < ns ? (hi_y < -1e9 ? (long)-1e9 : (long)hi_y) : ns;
        if (xmax <= xmin || ymax <= ymin) {
            if (mo_box_pixels(box[i]) != 0) bad_caps++;
            continue;
        }
        if (box[i].x0 != xmin || box[i].y0 != ymin || box[i].w != xmax - xmin || box[i].h != ymax - ymin) bad_caps++;
        for (long iy = ymin; iy < ymax; iy++)
            for (long ix = xmin; ix < xmax; ix++)
                if (hypot((double)ix - x[i], (double)iy - y[i]) < r[i]) plain.at((size_t)iy * ns + ix) = 1;
    }
    if (flat != plain || flat != want) bad_caps++;
}

static void decibel_job()
{
    const int type = (int)next(), divisor = (int)next();
    const float bels = (float)next_double();
    const long n = next();
    for (long i = 0; i < n; i++) {
        const int64_t code = next();
        const uint32_t want = (uint32_t)next();
        const uint8_t c8 = (uint8_t)code;
        const uint16_t c16 = (uint16_t)code;
        const int16_t s16 = (int16_t)code;
        const void *src = type == 0 ? (const void *)&c8 : type == 1 ? (const void *)&c16 : (const void *)&s16;
        const float v = mo_db(mo_code_value(src, type, 0), bels, divisor ? MO_NOISE_DIV : MO_FIDELITY_DIV);
        uint32_t got;
        memcpy(&got, &v, 4);
        float wv;
        memcpy(&wv, &want, 4);
        n_db++;
        if (got != want && !(v != v && wv != wv)) bad_db++;
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t w;
    while (fread(&w, 8, 1, f) == 1) words.push_back(w);
    fclose(f);
    const int64_t jobs = next();
    for (int64_t j = 0; j < jobs; j++) {
        const int64_t kind = next();
        if (kind == 0) window_job();
        else if (kind == 1) caps_job();
        else if (kind == 2) decibel_job();
        else return 2;
    }
    if (at != words.size()) return 2;
    printf("windows %ld %ld\nsplits %ld %ld\ncaps %ld %ld\npixels %ld %ld\ndecibels %ld %ld\n", n_windows, bad_windows, n_splits, bad_splits, n_caps, bad_caps, n_pixels,
           bad_pixels, n_db, bad_db);
    return (bad_windows || bad_splits || bad_caps || bad_pixels || bad_db) ? 1 : 0;
}
