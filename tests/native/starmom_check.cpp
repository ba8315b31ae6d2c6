// starmom_check.cpp -- the host-compilable core of csrc/starmom.hip (starmom_core.h).  argv[1]: a text dump of the iterations the golden
// generator recorded for some fixture stars (tests/test_starcat_host.py writes it from tests/golden/starcat.npz): per iteration the state
// before, the rows with their column ranges, the seven sums and the state after.  Checked are: the core's ranges against the recorded ones
// (exactly) and against a loop over every pixel of the cut that forms rho2 directly; the core's pixel sums against the recorded sums; the
// core's step on the recorded sums against the recorded next state; and, with synthetic sums, every way the iteration can end, the
// 400-iteration cap included.  Prints one line a check, "<what> <comparisons> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "starmom_core.h"

using namespace imcom;

static const imcom_star_params P = {1e-6, 0.25, 8000.0, 15.0, 25.0, 5.0, 400, 0};
static long total_fails = 0;

static void report(const char *what, long checks, long fails)
{
    printf("%s %ld %ld\n", what, checks, fails);
    total_fails += fails;
}

static bool close_to(double a, double b, double scale, double tol) { return (a != a && b != b) || std::fabs(a - b) <= tol * scale; }

static void check_dump(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        printf("cannot open %s\n", path);
        exit(2);
    }
    long range_checks = 0, range_fails = 0, brute_checks = 0, brute_fails = 0, sum_checks = 0, sum_fails = 0, step_checks = 0, step_fails = 0;
    int ntraces = 0;
    if (fscanf(f, "N %d", &ntraces) != 1) exit(2);
    for (int t = 0; t < ntraces; t++) {
        int h, w, niter;
        if (fscanf(f, " T %d %d %d", &h, &w, &niter) != 3) exit(2);
        std::vector<double> img((size_t)h * w);
        for (double &v : img)
            if (fscanf(f, "%lf", &v) != 1) exit(2);
        for (int it = 0; it < niter; it++) {
            SmState s;
            sm_init(s, w, h, P);
            int nrows;
            if (fscanf(f, " P %lf %lf %lf %lf %lf %lf %d %d", &s.x0, &s.y0, &s.Mxx, &s.Mxy, &s.Myy, &s.shiftscale0, &s.iter, &nrows) != 8) exit(2);
            std::vector<int> riy(nrows), rx1(nrows), rx2(nrows);
            for (int r = 0; r < nrows; r++)
                if (fscanf(f, " R %d %d %d", &riy[r], &rx1[r], &rx2[r]) != 3) exit(2);
            double want[SM_NSUMS], after[5], cf;
            int status;
            if (fscanf(f, " S %lf %lf %lf %lf %lf %lf %lf", want, want + 1, want + 2, want + 3, want + 4, want + 5, want + 6) != 7) exit(2);
            if (fscanf(f, " Q %lf %lf %lf %lf %lf %lf %d", after, after + 1, after + 2, after + 3, after + 4, &cf, &status) != 7) exit(2);
            // the ranges, and the sums by the core's own pixel function
            int iy1, iy2, r = 0;
            range_checks++;
            if (!sm_begin(s, h, P, &iy1, &iy2)) {
                range_fails++;
                continue;
            }
            double sum[SM_NSUMS] = {0, 0, 0, 0, 0, 0, 0}, mag[SM_NSUMS] = {0, 0, 0, 0, 0, 0, 0};
            std::vector<char> inside((size_t)h * w, 0);
            for (int iy = iy1; iy <= iy2; iy++) {
                double dy, b;
                int ix1, ix2;
                if (!sm_row(s, iy, w, P, &dy, &b, &ix1, &ix2)) continue;
                range_checks++;
                if (r >= nrows || riy[r] != iy || rx1[r] != ix1 || rx2[r] != ix2) range_fails++;
                r++;
                for (int ix = ix1; ix <= ix2; ix++) {
                    const double v = img[(size_t)(iy - 1) * w + ix - 1];
                    sm_pixel(s, ix, dy, b, v, sum);
                    sm_pixel(s, ix, dy, b, std::fabs(v), mag);  // (mag[0]: the sum of the weights' magnitudes)
                    inside[(size_t)(iy - 1) * w + ix - 1] = 1;
                }
            }
            range_checks++;
            range_fails += r != nrows;
            // a straightforward loop: every pixel, rho2 from M's inverse
            for (int iy = 1; iy <= h; iy++)
                for (int ix = 1; ix <= w; ix++) {
                    const double dx = ix - s.x0, dy = iy - s.y0;
                    const double rho2 = (s.Myy * dx * dx - 2.0 * s.Mxy * dx * dy + s.Mxx * dy * dy) / s.detM;
                    if (std::fabs(rho2 - P.max_moment_nsig2) < 1e-9 * P.max_moment_nsig2) continue;  // (on the edge: either answer)
                    brute_checks++;
                    brute_fails += (rho2 < P.max_moment_nsig2) != (bool)inside[(size_t)(iy - 1) * w + ix - 1];
                }
            for (int i = 0; i < SM_NSUMS; i++) {
                sum_checks++;
                const double lever = i == 0 ? 1.0 : i < 3 ? (double)(w + h) : i < 6 ? (double)(w + h) * (double)(w + h) : P.max_moment_nsig2 * P.max_moment_nsig2;
                sum_fails += !close_to(sum[i], want[i], mag[0] * lever, 1e-12);  // (a term is at most its weight times a power of the offset)
            }
            // the step on the recorded sums
            const bool go = sm_step(s, want, P);
            step_checks += 7;
            step_fails += (go ? -1 : s.status) != status;
            step_fails += !close_to(s.x0, after[0], std::fabs(after[0]), 1e-13) + !close_to(s.y0, after[1], std::fabs(after[1]), 1e-13);
            const double ms = std::fabs(after[2]) + std::fabs(after[4]);
            step_fails += !close_to(s.Mxx, after[2], ms, 1e-13) + !close_to(s.Mxy, after[3], ms, 1e-13) + !close_to(s.Myy, after[4], ms, 1e-13);
            step_fails += !close_to(s.cf, cf, std::fabs(cf), 1e-9);  // (the factor is a difference of nearly equal numbers near the end)
        }
    }
    fclose(f);
    report("ranges recorded", range_checks, range_fails);
    report("ranges brute", brute_checks, brute_fails);
    report("sums recorded", sum_checks, sum_fails);
    report("step recorded", step_checks, step_fails);
}

// sums that leave the state where it is: B = 0, C = M A / 2
static void neutral(const SmState &s, double A, double *sum)
{
    sum[0] = A, sum[1] = sum[2] = 0.0, sum[3] = 0.5 * s.Mxx * A, sum[4] = 0.5 * s.Mxy * A, sum[5] = 0.5 * s.Myy * A, sum[6] = 2.0 * A;
}

static void check_endings()
{
    long checks = 0, fails = 0;
    int iy1, iy2;
    double sum[SM_NSUMS];
    SmState s;
    // converged at once
    sm_init(s, 79, 79, P);
    fails += !sm_begin(s, 79, P, &iy1, &iy2) || iy1 != 15 || iy2 != 65;
    neutral(s, 1.5, sum);
    fails += sm_step(s, sum, P) || s.status != SM_OK || s.iter != 1 || s.cf != 0.0;
    double col[SM_NCOL] = {0};
    sm_finish(s, sum, col);
    fails += col[SMC_AMP] != 3.0 || col[SMC_X] != 40.0 || std::fabs(col[SMC_SIGMA] - 5.0) > 1e-14 || col[SMC_E1] != 0.0 || col[SMC_G2] != 0.0 || col[SMC_RHO4] != 2.0;
    checks += 3;
    // even sides: a half-integer start
    sm_init(s, 12, 10, P);
    fails += s.x0 != 6.5 || s.y0 != 5.5;
    checks++;
    // not positive definite: at the head, and through semi_b2
    sm_init(s, 31, 31, P);
    s.Mxy = 30.0;
    fails += sm_begin(s, 31, P, &iy1, &iy2) || s.status != SM_NOT_POSITIVE_DEFINITE;
    sm_init(s, 31, 31, P);
    s.Mxx = 0.0 / 1.0 - 1.0;
    fails += sm_begin(s, 31, P, &iy1, &iy2) || s.status != SM_NOT_POSITIVE_DEFINITE;
    sm_init(s, 31, 31, P);
    s.Mxx = std::nan("");
    fails += sm_begin(s, 31, P, &iy1, &iy2) || s.status != SM_NOT_POSITIVE_DEFINITE;
    checks += 3;
    // empty bounds: the centroid far off the image
    sm_init(s, 31, 31, P);
    s.y0 = -100.0;
    fails += sm_begin(s, 31, P, &iy1, &iy2) || s.status != SM_EMPTY_BOUNDS;
    sm_init(s, 31, 31, P);
    s.x0 = 200.0;
    {
        double dy, b;
        int ix1, ix2;
        fails += !sm_begin(s, 31, P, &iy1, &iy2) || sm_row(s, 16, 31, P, &dy, &b, &ix1, &ix2);
    }
    checks += 2;
    // a shift too large: the centroid pushed a quarter of the shift scale a step
    sm_init(s, 79, 79, P);
    int n = 0;
    for (; n < 1000; n++) {
        neutral(s, 1.0, sum);
        sum[1] = 1e9;
        if (!sm_step(s, sum, P)) break;
    }
    fails += s.status != SM_TOO_LARGE || n != 12 || s.x0 - s.x00 != 16.25;  // (13 steps of 1.25)
    // a moment too large: the moments grown by a quarter of semi_b2 a step
    sm_init(s, 79, 79, P);
    for (n = 0; n < 1000; n++) {
        neutral(s, 1.0, sum);
        sum[3] = sum[5] = 1e12;
        if (!sm_step(s, sum, P)) break;
    }
    fails += s.status != SM_TOO_LARGE || !(s.Mxx > P.max_amoment) || n > 40;
    checks += 2;
    // too many iterations: the centroid pushed to and fro for ever
    sm_init(s, 79, 79, P);
    for (n = 0; n < 1000; n++) {
        neutral(s, 1.0, sum);
        sum[1] = (n & 1) ? -1e9 : 1e9;
        if (!sm_step(s, sum, P)) break;
    }
    fails += s.status != SM_TOO_MANY_ITERATIONS || s.iter != P.max_mom2_iter + 1 || n != P.max_mom2_iter;
    checks++;
    // NaN: an all-zero cut divides by A = 0; a NaN among the data
    sm_init(s, 15, 15, P);
    for (int i = 0; i < SM_NSUMS; i++) sum[i] = 0.0;
    fails += sm_step(s, sum, P) || s.status != SM_NAN || s.iter != 1;
    sm_init(s, 15, 15, P);
    for (int i = 0; i < SM_NSUMS; i++) sum[i] = std::nan("");
    fails += sm_step(s, sum, P) || s.status != SM_NAN;
    checks += 2;
    report("endings synthetic", checks, fails);
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        printf("usage: starmom_check <dump>\n");
        return 2;
    }
    check_dump(argv[1]);
    check_endings();
    return total_fails ? 1 : 0;
}
