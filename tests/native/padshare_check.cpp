// padshare_check.cpp -- csrc/padshare_core.h as a host program (built with -fsanitize=address,undefined by tests/test_padshare_host.py).
// Reads a file of 64-bit words: the number of jobs, then per job (planes are n x n, one element a word, float32 as its bits)
//   0, direction, add_mode, n, w, fk, mine, theirs, expected                           a PRIMARY plane
//   1, direction, add_mode, n, w, fk, bits of the decode coefficient, floor code, encode coefficient, unsigned,
//      mine, theirs, expected codes, (w + fk) n expected float32 sums of my strip      a quality map plane
//   2, direction, n1P, pad, mine, theirs, expected                                     an INWEIGHT plane
// Every plane is updated as the kernels of csrc/block.hip update it -- strip pixel t to its position and the two offsets, then the core's
// arithmetic -- and compared as a whole: what lies outside my strip must not change.  Prints "<what> <checked> <failures>" for layers,
// maps, sums and weights; exit status 1 on any failure.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "padshare_core.h"

using namespace imcom;

static std::vector<int64_t> words;
static size_t at = 0;
static int64_t next() { return words.at(at++); }
static float as_float(int64_t w)
{
    const uint32_t u = (uint32_t)w;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static bool same(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

static long n_layers = 0, bad_layers = 0, n_maps = 0, bad_maps = 0, n_sums = 0, bad_sums = 0, n_weights = 0, bad_weights = 0;

// block.hip's padshare_pixel
static void pixel(int direction, const PsStrip &s, int n, long t, int *p, long *mo, long *uo)
{
    if (ps_along_x(direction)) {
        const int y = (int)(t / s.len);
        *p = (int)(t - (long)y * s.len);
        *mo = (long)y * n + s.my0 + *p;
        *uo = (long)y * n + s.ur0 + *p;
    } else {
        *p = (int)(t / n);
        const int x = (int)(t - (long)*p * n);
        *mo = (long)(s.my0 + *p) * n + x;
        *uo = (long)(s.ur0 + *p) * n + x;
    }
}

static std::vector<float> float_plane(size_t count)
{
    std::vector<float> v(count);
    for (auto &x : v) x = as_float(next());
    return v;
}

static void layers_job()
{
    const int direction = (int)next(), add = (int)next(), n = (int)next(), w = (int)next(), fk = (int)next();
    if (!ps_shape_ok(direction, n, w, fk)) { bad_layers++; return; }
    std::vector<float> mine = float_plane((size_t)n * n), theirs = float_plane((size_t)n * n), want = float_plane((size_t)n * n);
    const PsStrip s = ps_strip(direction, n, w, fk);
    for (long t = 0; t < (long)s.len * n; t++) {
        int p;
        long mo, uo;
        pixel(direction, s, n, t, &p, &mo, &uo);
        mine.at(mo) = ps_combine(mine.at(mo), theirs.at(uo), add);
    }
    for (size_t i = 0; i < mine.size(); i++) {
        n_layers++;
        if (!same(mine[i], want[i])) bad_layers++;
    }
}

static void map_job()
{
    const int direction = (int)next(), add = (int)next(), n = (int)next(), w = (int)next(), fk = (int)next();
    const int64_t cb = next();
    double coef;
    memcpy(&coef, &cb, 8);
    const int floor_code = (int)next(), encode_coef = (int)next(), uns = (int)next();
    if (!ps_shape_ok(direction, n, w, fk)) { bad_maps++; return; }
    std::vector<uint16_t> mine((size_t)n * n), theirs((size_t)n * n), want((size_t)n * n);
    for (auto &x : mine) x = (uint16_t)next();
    for (auto &x : theirs) x = (uint16_t)next();
    for (auto &x : want) x = (uint16_t)next();
    const PsStrip s = ps_strip(direction, n, w, fk);
    std::vector<float> sums = float_plane((size_t)s.len * n);
    for (long t = 0; t < (long)s.len * n; t++) {
        int p;
        long mo, uo;
        pixel(direction, s, n, t, &p, &mo, &uo);
        float mv = ps_decode(ps_code(mine.at(mo), uns), coef, floor_code), uv = ps_decode(ps_code(theirs.at(uo), uns), coef, floor_code);
        if (add) {
            const int km = ps_taper_mine(direction, p, w, fk), ku = ps_taper_theirs(direction, p, w, fk);
            if (km >= 2 * fk || ku >= 2 * fk || (km >= 0) != (ku >= 0) || (km >= 0 && km + ku != 2 * fk - 1)) bad_maps++;  // the two fades are complementary
            mv = ps_taper(mv, km, fk);
            uv = ps_taper(uv, ku, fk);
        }
        const float sum = ps_combine(mv, uv, add);
        n_sums++;
        if (!same(sum, sums.at(t))) bad_sums++;
        mine.at(mo) = ps_encode(sum, (float)encode_coef, uns);
    }
    for (size_t i = 0; i < mine.size(); i++) {
        n_maps++;
        if (mine[i] != want[i]) bad_maps++;
    }
}

static void weights_job()
{
    const int direction = (int)next(), n1P = (int)next(), pad = (int)next();
    if (!ps_shape_ok(direction, n1P, pad, 0)) { bad_weights++; return; }
    std::vector<float> mine = float_plane((size_t)n1P * n1P), theirs = float_plane((size_t)n1P * n1P), want = float_plane((size_t)n1P * n1P);
    const PsStrip s = ps_strip(direction, n1P, pad, 0);
    for (long t = 0; t < (long)s.len * n1P; t++) {
        int p;
        long mo, uo;
        pixel(direction, s, n1P, t, &p, &mo, &uo);
        mine.at(mo) = theirs.at(uo);
    }
    for (size_t i = 0; i < mine.size(); i++) {
        n_weights++;
        if (!same(mine[i], want[i])) bad_weights++;
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
        if (kind == 0) layers_job();
        else if (kind == 1) map_job();
        else if (kind == 2) weights_job();
        else return 2;
    }
    if (at != words.size()) return 2;
    // shapes that every entry refuses
    if (ps_shape_ok(4, 32, 8, 2) || ps_shape_ok(-1, 32, 8, 2) || ps_shape_ok(0, 32, 1, 2) || ps_shape_ok(0, 15, 8, 0) || !ps_shape_ok(3, 16, 8, 8)) bad_layers++;
    printf("layers %ld %ld\nmaps %ld %ld\nsums %ld %ld\nweights %ld %ld\n", n_layers, bad_layers, n_maps, bad_maps, n_sums, bad_sums, n_weights, bad_weights);
    return (bad_layers || bad_maps || bad_sums || bad_weights) ? 1 : 0;
}
