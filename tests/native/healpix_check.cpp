// healpix_check.cpp -- csrc/healpix_core.h as a host program (g++ -fsanitize=address,undefined; tests/test_healpix_host.py builds and runs it).
// argv[1]: a file of int64 values (float64 values as their bit patterns) written by the test from tests/golden/healpix.npz:
//   number of jobs, then a job each:
//   kind 0 (pixels): n, bound of theta, bound of phi, then n times (res, pixel, exact theta, exact phi)
//   kind 1 (cap):    res, ra, dec, radius, mode (0 the reference's range, 1 the full disc), n, then the n expected pixels, ascending
// Pixels: |core - exact| <= bound per angle; ang2pix of the exact centre is the pixel; ring, start and length agree with the pixel.
// Caps: the rings of the range through their phi windows, as the kernel walks them, give exactly the expected pixels in ascending order;
// up to res 6 every pixel of the sphere is tested too, so a window that is too narrow shows.
// Then, without the file's help: the integer square root around every kind of boundary, the window traversal, the box, the position angle.
// Prints a line "name checked failures" a part; the exit status is the number of parts with failures.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "healpix_core.h"

using namespace imcom;

static std::vector<int64_t> read_all(const char *path)
{
    std::vector<int64_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(99);
    }
    int64_t buf[4096];
    size_t k;
    while ((k = fread(buf, 8, 4096, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static double as_double(int64_t b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}

static int report(const char *name, long checked, long failures)
{
    printf("%s %ld %ld\n", name, checked, failures);
    return failures != 0;
}

// The cap as the kernel forms it: ring by ring, each ring's window in ascending index.
static std::vector<int64_t> cap_by_windows(int res, double ra, double dec, double radius, int mode, long *tested)
{
    int64_t pmin, pmax;
    hp_cap_range(res, ra, dec, radius, &pmin, &pmax);
    HpRing g0, g1;
    hp_ring_info(res, hp_pix2ring(res, pmin), &g0);
    hp_ring_info(res, hp_pix2ring(res, pmax), &g1);
    const int64_t plo = mode ? g0.start : pmin, phi_ = mode ? g1.start + g1.len - 1 : pmax;
    const double sd = sin(dec), cd = cos(dec), cosr = cos(radius), theta0 = HP_HALFPI - dec, s0 = cd > 0.0 ? cd : 0.0, raw = hp_fmodulo(ra, HP_TWOPI);
    std::vector<int64_t> out;
    for (int64_t r = g0.ring; r <= g1.ring; r++) {
        HpRing g;
        hp_ring_info(res, r, &g);
        double z, sth;
        const double theta = hp_ring_theta(res, r, &z, &sth);
        int64_t first, count;
        hp_ring_window(theta, sth, theta0, s0, radius, raw, g, &first, &count);
        for (int64_t k = 0; k < count; k++) {
            const int64_t j = hp_window_index(g, first, count, k), p = g.start + j;
            if (j < 0 || j >= g.len) {
                out.push_back(-1);  // (a failure whatever is expected)
                continue;
            }
            if (p < plo || p > phi_) continue;
            ++*tested;
            if (hp_cap_mu(sd, cd, ra, theta, hp_ring_phi(g, j)) >= cosr) out.push_back(p);
        }
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 98;
    const std::vector<int64_t> v = read_all(argv[1]);
    size_t at = 0;
    const long njobs = (long)v[at++];
    int bad_parts = 0;
    long pix_checked = 0, pix_failures = 0, cap_checked = 0, cap_failures = 0, tested = 0;
    double worst = 0.0;
    for (long job = 0; job < njobs; job++) {
        const int kind = (int)v[at++];
        if (kind == 0) {
            const long n = (long)v[at++];
            const double bt = as_double(v[at]), bp = as_double(v[at + 1]);
            at += 2;
            for (long i = 0; i < n; i++, at += 4) {
                const int res = (int)v[at];
                const int64_t p = v[at + 1];
                const double et = as_double(v[at + 2]), ep = as_double(v[at + 3]);
                double theta, phi;
                hp_pix2ang(res, p, &theta, &phi);
                HpRing g;
                hp_ring_info(res, hp_pix2ring(res, p), &g);
                bool ok = fabs(theta - et) <= bt && fabs(phi - ep) <= bp && phi >= 0.0 && phi < HP_TWOPI;
                ok = ok && hp_ang2pix(res, et, ep) == p && hp_ang2pix(res, theta, phi + HP_TWOPI) == p && hp_ang2pix(res, theta, phi - 3.0 * HP_TWOPI) == p;
                ok = ok && p >= g.start && p < g.start + g.len && g.ring >= 1 && g.ring <= 4 * hp_nside(res) - 1;
                pix_checked++;
                if (!ok) pix_failures++;
                if (fabs(theta - et) / bt > worst) worst = fabs(theta - et) / bt;
                if (fabs(phi - ep) / bp > worst) worst = fabs(phi - ep) / bp;
            }
        } else {
            const int res = (int)v[at];
            const double ra = as_double(v[at + 1]), dec = as_double(v[at + 2]), radius = as_double(v[at + 3]);
            const int mode = (int)v[at + 4];
            const long n = (long)v[at + 5];
            at += 6;
            const std::vector<int64_t> got = cap_by_windows(res, ra, dec, radius, mode, &tested);
            bool ok = (long)got.size() == n;
            for (long i = 0; ok && i < n; i++) ok = got[i] == v[at + i] && (i == 0 || got[i] > got[i - 1]);
            if (ok && mode == 1 && res <= 6) {  // every pixel of the sphere
                long hits = 0;
                const double sd = sin(dec), cd = cos(dec), cosr = cos(radius);
                for (int64_t p = 0; p < hp_npix(res); p++) {
                    double theta, phi;
                    hp_pix2ang(res, p, &theta, &phi);
                    if (hp_cap_mu(sd, cd, ra, theta, phi) >= cosr) hits++;
                }
                ok = hits == n;
            }
            at += n;
            cap_checked++;
            if (!ok) cap_failures++;
        }
    }
    bad_parts += report("pixels", pix_checked, pix_failures);
    bad_parts += report("caps", cap_checked, cap_failures);
    fprintf(stderr, "largest error / bound over the pixels: %.3f; %ld candidates tested in the caps\n", worst, tested);

    // the integer square root: squares, their neighbours, the largest argument of the scheme
    long checked = 0, failures = 0;
    {
        const uint64_t roots[] = {0, 1, 2, 3, 94906265, 94906266, 94906267, 2147483647ull, 2147483648ull, 2626999999ull, 2627413513ull, 3037000499ull};
        for (uint64_t r : roots) {
            for (int d = -2; d <= 2; d++) {
                const uint64_t sq = r * r;
                if (d < 0 && sq < (uint64_t)(-d)) continue;
                const uint64_t a = sq + d, got = hp_isqrt(a);
                checked++;
                if (!(got * got <= a && (got + 1) * (got + 1) > a)) failures++;
            }
        }
        const uint64_t top = 2ull * 12ull << 58;  // 2 * 12 * 4^29
        checked++;
        if (!(hp_isqrt(top) * hp_isqrt(top) <= top && (hp_isqrt(top) + 1) * (hp_isqrt(top) + 1) > top)) failures++;
        // every ring boundary of res 10: the first and last pixel of every ring
        for (int64_t r = 1; r <= 4 * hp_nside(10) - 1; r++) {
            HpRing g;
            hp_ring_info(10, r, &g);
            checked += 2;
            if (hp_pix2ring(10, g.start) != r) failures++;
            if (hp_pix2ring(10, g.start + g.len - 1) != r) failures++;
            if (r == 4 * hp_nside(10) - 1 && g.start + g.len != hp_npix(10)) failures++;
        }
    }
    bad_parts += report("integers", checked, failures);

    // the window: empty, whole, wrapped; the traversal ascends and stays inside the ring
    checked = failures = 0;
    {
        HpRing g;
        hp_ring_info(5, 40, &g);
        double z, sth;
        const double theta = hp_ring_theta(5, 40, &z, &sth);
        int64_t first, count;
        hp_ring_window(theta, sth, theta + 0.5, sin(theta + 0.5), 0.3, 1.0, g, &first, &count);
        checked++;
        if (count != 0) failures++;
        hp_ring_window(theta, sth, 0.0, 0.0, 3.0, 1.0, g, &first, &count);  // a cap about the pole
        checked++;
        if (count != g.len || first != 0) failures++;
        hp_ring_window(theta, sth, theta, sth, 0.2, 0.01, g, &first, &count);  // across phi = 0
        checked++;
        if (!(count > 2 && count < g.len && first + count > g.len)) failures++;
        int64_t last = -1;
        for (int64_t k = 0; k < count; k++) {
            const int64_t j = hp_window_index(g, first, count, k);
            checked++;
            if (!(j > last && j < g.len)) failures++;
            last = j;
        }
        hp_ring_window(theta, sth, theta, sth, NAN, 0.01, g, &first, &count);  // (refused by the entry; here: no index leaves the ring)
        checked++;
        if (!(count >= 0 && count <= g.len && first >= 0 && first < g.len)) failures++;
    }
    bad_parts += report("windows", checked, failures);

    // the box and the position angle
    checked = failures = 0;
    {
        checked += 7;
        if (!hp_in_box(39.5, 200, 40)) failures++;  // rint = 40: halves go to the even neighbour
        if (hp_in_box(38.5, 200, 40)) failures++;   // rint = 38
        if (!hp_in_box(159.49, 200, 40)) failures++;
        if (hp_in_box(159.5, 200, 40)) failures++;  // rint = 160
        if (hp_in_box(NAN, 200, 40)) failures++;
        if (hp_in_box(40000.0, 70000, 40)) failures++;  // does not fit int16
        if (hp_in_box(-INFINITY, 200, 40)) failures++;
        checked += 4;
        if (fabs(hp_position_angle(1.0, 0.0, -1.0, 0.0) - 90.0) > 1e-13) failures++;
        if (fabs(hp_position_angle(-1.0, 0.0, 1.0, 0.0) - 270.0) > 1e-13) failures++;
        if (hp_position_angle(0.0, 1.0, 0.0, -1.0) != 0.0) failures++;
        const double pa = hp_position_angle(-1e-300, 1.0, 0.0, -1.0);
        if (!(pa >= 0.0 && pa < 360.0)) failures++;
    }
    bad_parts += report("box", checked, failures);
    return bad_parts;
}
