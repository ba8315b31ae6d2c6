// wcs_check.cpp -- csrc/wcs_core.h as a host program (g++ -fsanitize=address,undefined; tests/test_wcs_host.py builds and runs it).
// argv[1]: a file of float64 values written by the test from tests/golden/wcs.npz:
//   n2, lo, hi, table as float64 [2][n2][n2], the float32 table widened to float64 [2][n2][n2], number of jobs, then a job each:
//   kind (0 pixel -> world, 1 world -> pixel, 2 pixel -> pixel), origin, n, bound of the first output, bound of the second,
//   table of a (0 none, 1 float32, 2 float64), descriptor a [130], table of b, descriptor b [130], inputs [n][2], expected [n][2]
// Every job: |core - expected| <= bound per output (ra on the circle).  Then, without the file's help: the cell search at every node, in
// every cell and beyond both ends against a plain scan of the node list; the Newton cap; the NaN exits.
// Prints a line "name checked failures" a part; the exit status is the number of parts with failures.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wcs_core.h"

using namespace imcom;

static std::vector<double> read_all(const char *path)
{
    std::vector<double> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(99);
    }
    double buf[4096];
    size_t k;
    while ((k = fread(buf, 8, 4096, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static int report(const char *name, long checked, long failures)
{
    printf("%s %ld %ld\n", name, checked, failures);
    return failures != 0;
}

static WcsDesc plain_tan(double sip_a20)
{
    WcsDesc w = {};
    w.d[WCS_D_PROJ] = WCS_TAN;
    w.d[WCS_D_CRPIX] = w.d[WCS_D_CRPIX + 1] = 100.5;
    w.d[WCS_D_CD] = -3e-5, w.d[WCS_D_CD + 3] = 3e-5;
    // CRVAL = (0, 0), LONPOLE = 180 in Paper II eq. (2): sa = sd = sp = 0, ca = cd = 1, cp = -1
    const double R2[9] = {0, 0, -1, 0, 1, 0, 1, 0, 0};
    for (int k = 0; k < 9; k++) w.d[WCS_D_ROT + k] = R2[k];
    if (sip_a20 != 0.0) {
        w.d[WCS_D_AORDER] = 2;
        w.d[WCS_D_A + wcs_sip_index(2, 0)] = sip_a20;
    }
    return w;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 98;
    const std::vector<double> v = read_all(argv[1]);
    size_t at = 0;
    const int n2 = (int)v[at++];
    const double lo = v[at++], hi = v[at++];
    const size_t tn = (size_t)2 * n2 * n2;
    std::vector<double> t64(v.begin() + at, v.begin() + at + tn);
    at += tn;
    std::vector<float> t32(tn);
    for (size_t k = 0; k < tn; k++) t32[k] = (float)v[at + k];
    at += tn;
    const WcsTab tabs[3] = {{nullptr, 0, 0, 0.0, 0.0}, {t32.data(), 0, n2, lo, hi}, {t64.data(), 1, n2, lo, hi}};
    const int njobs = (int)v[at++];
    int bad_parts = 0;
    long checked = 0, failures = 0;
    double worst = 0.0;
    for (int j = 0; j < njobs; j++) {
        const int kind = (int)v[at++], origin = (int)v[at++];
        const long n = (long)v[at++];
        const double b0 = v[at++], b1 = v[at++];
        WcsDesc a, b;
        const WcsTab &ta = tabs[(int)v[at++]];
        for (int k = 0; k < WCS_DESC_LEN; k++) a.d[k] = v[at++];
        const WcsTab &tb = tabs[(int)v[at++]];
        for (int k = 0; k < WCS_DESC_LEN; k++) b.d[k] = v[at++];
        const double *in = &v[at], *ex = &v[at + 2 * n];
        at += 4 * n;
        double M[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s += b.d[WCS_D_ROT + 3 * r + k] * a.d[WCS_D_ROT + 3 * c + k];
                M[3 * r + c] = s;
            }
        for (long i = 0; i < n; i++) {
            double o0, o1;
            bool ok = true;
            if (kind == 0) wcs_pix2world(a, ta, in[2 * i], in[2 * i + 1], origin, &o0, &o1);
            else if (kind == 1) ok = wcs_world2pix(a, ta, in[2 * i], in[2 * i + 1], origin, &o0, &o1);
            else ok = wcs_pix2pix(a, ta, b, tb, M, in[2 * i], in[2 * i + 1], origin, &o0, &o1);
            double e0 = fabs(o0 - ex[2 * i]);
            const double e1 = fabs(o1 - ex[2 * i + 1]);
            if (kind == 0) {
                if (e0 > 180.0) e0 = 360.0 - e0;
                if (!(o0 >= 0.0 && o0 < 360.0)) ok = false;
            }
            checked++;
            if (!ok || !(e0 <= b0) || !(e1 <= b1)) failures++;
            if (e0 / b0 > worst) worst = e0 / b0;
            if (e1 / b1 > worst) worst = e1 / b1;
        }
    }
    bad_parts += report("fixture", checked, failures);
    fprintf(stderr, "largest error / bound over the fixture: %.3f\n", worst);

    // the cell search: every node, the middle of every cell, one ulp either side of every node, far beyond both ends
    checked = failures = 0;
    std::vector<double> nodes(n2);
    for (int k = 0; k < n2; k++) nodes[k] = wcs_tab_node(k, n2, lo, hi);
    std::vector<double> probes = {lo - 1e6, lo - 1.0, hi + 1.0, hi + 1e6, -0.0};
    for (int k = 0; k < n2; k++) {
        probes.push_back(nodes[k]);
        probes.push_back(nextafter(nodes[k], -INFINITY));
        probes.push_back(nextafter(nodes[k], INFINITY));
        if (k + 1 < n2) probes.push_back(0.5 * (nodes[k] + nodes[k + 1]));
    }
    for (double t : probes) {
        int want = 0;  // the last i <= n2 - 2 with nodes[i] <= t, 0 below the first node
        for (int i = 0; i <= n2 - 2; i++)
            if (nodes[i] <= t) want = i;
        double f;
        const int got = wcs_tab_cell(t, n2, lo, hi, &f);
        const double fw = (t - nodes[want]) / (nodes[want + 1] - nodes[want]);
        checked++;
        if (got != want || f != fw) failures++;
        // and the gather stays inside the table for every probe pair
        double dx, dy;
        wcs_tab_offsets(tabs[1], t, -t, &dx, &dy);
        wcs_tab_offsets(tabs[2], -t, t, &dx, &dy);
        if (!(dx - dx == 0.0 && dy - dy == 0.0)) failures++;
    }
    bad_parts += report("cells", checked, failures);

    // the Newton cap: u + u^2 = U has no real solution for U < -1/4 -> not stopped -> NaN; a mild polynomial stops
    checked = failures = 0;
    {
        const WcsDesc hard = plain_tan(1.0), mild = plain_tan(1e-6);
        double x, y;
        // native vector of the pixel 2000 columns left of CRPIX under the linear part: U = -2000
        double xi, eta, n[3];
        const WcsDesc lin = plain_tan(0.0);
        wcs_pix2inter(lin, 100.5 - 1.0 - 2000.0, 50.0, 0, &xi, &eta);
        wcs_inter2native(WCS_TAN, xi, eta, n);
        checked++;
        if (wcs_native2pix(hard, n, 0, &x, &y) || x == x || y == y) failures++;
        checked++;
        if (!wcs_native2pix(mild, n, 0, &x, &y) || !(fabs((x - 99.5) + 1e-6 * (x - 99.5) * (x - 99.5) + 2000.0) < 1e-8)) failures++;
        checked++;
        if (!wcs_native2pix(lin, n, 0, &x, &y) || !(fabs(x + 1900.5) < 1e-8 && fabs(y - 50.0) < 1e-8)) failures++;
    }
    // far off the chip, where an ulp of the coordinate exceeds 2^-40 pixel: every point stops (a test on the step alone can alternate
    // between the two neighbours of the root for ever) and solves its equation to an ulp
    {
        const WcsDesc mild = plain_tan(-3e-7);
        for (int k = 0; k < 40000; k++) {
            const double U = 4096.0 + 0.30717 * k, n[3] = {0.0, -3e-5 * WCS_DEG * U, 1.0};  // xi = CD1_1 U, eta = 0, up to the normalisation
            double x, y;
            checked++;
            const bool ok = wcs_native2pix(mild, n, 0, &x, &y);
            const double u = x - 99.5;
            if (!ok || !(fabs((u - U) - 3e-7 * u * u) < 4.0 * 2.220446049250313e-16 * U)) failures++;
        }
    }
    bad_parts += report("newton", checked, failures);

    // the NaN exits
    checked = failures = 0;
    {
        WcsDesc tan = plain_tan(0.0), stg = plain_tan(0.0);
        stg.d[WCS_D_PROJ] = WCS_STG;
        double x, y;
        const double far[3] = {0.3, 0.1, -0.2}, edge[3] = {1.0, 0.0, 0.0}, anti[3] = {0.0, 0.0, -1.0}, nanv[3] = {NAN, 0.0, 1.0}, infv[3] = {INFINITY, 0.0, 1.0},
                     pole[3] = {0.0, 0.0, 1.0};
        checked += 7;
        if (wcs_native2pix(tan, far, 0, &x, &y) || x == x || y == y) failures++;
        if (wcs_native2pix(tan, edge, 0, &x, &y) || x == x) failures++;
        if (wcs_native2pix(stg, anti, 0, &x, &y) || x == x) failures++;
        if (!wcs_native2pix(stg, far, 0, &x, &y) || x != x) failures++;  // the far hemisphere is STG's to serve
        if (wcs_native2pix(tan, nanv, 0, &x, &y) || x == x) failures++;
        if (wcs_native2pix(stg, infv, 0, &x, &y) || x == x) failures++;
        if (!wcs_native2pix(tan, pole, 1, &x, &y) || x != 100.5 || y != 100.5) failures++;  // r = 0: CRPIX itself
        // through the whole chain: the antipode of CRVAL, NaN world coordinates, NaN pixels with and without a table
        checked += 5;
        if (wcs_world2pix(tan, tabs[0], 180.0, 0.0, 0, &x, &y) || x == x) failures++;
        if (wcs_world2pix(tan, tabs[0], NAN, 0.0, 0, &x, &y) || x == x) failures++;
        double ra, dec;
        wcs_pix2world(tan, tabs[2], NAN, 3.0, 0, &ra, &dec);
        if (ra == ra || dec == dec) failures++;
        wcs_pix2world(tan, tabs[0], 3.0, INFINITY, 0, &ra, &dec);
        if (ra == ra && dec == dec && !(ra >= 0.0 && ra < 360.0)) failures++;
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (wcs_pix2pix(tan, tabs[1], tan, tabs[1], I, NAN, NAN, 0, &x, &y) || x == x) failures++;
        // is_in_ref: strict in x, not in y; NaN outside
        checked += 5;
        if (wcs_is_in_ref(-0.5, 10.0, 64.0, 0.0)) failures++;
        if (!wcs_is_in_ref(10.0, -0.5, 64.0, 0.0)) failures++;
        if (!wcs_is_in_ref(nextafter(-3.5, 0.0), 63.5 + 3.0, 64.0, 3.0)) failures++;
        if (wcs_is_in_ref(10.0, nextafter(-3.5, -10.0), 64.0, 3.0)) failures++;
        if (wcs_is_in_ref(NAN, 1.0, 64.0, 0.0)) failures++;
    }
    bad_parts += report("exits", checked, failures);
    return bad_parts;
}
