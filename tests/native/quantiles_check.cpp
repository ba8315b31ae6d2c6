// quantiles_check.cpp -- the host-compilable core of csrc/quantiles.hip (quantiles_core.h) against the standard library: the walk down the
// digits with many ranks at once and the grouping of ranks by prefix against std::sort, the ring of a pixel and the clipped box of a star
// against integer arithmetic.  Prints one line a check, "<what> <type> <comparisons> <failures>"; exit status 1 on any failure.
#include <cstdio>
#include <limits>
#include <random>

#include "quantiles_core.h"

using namespace imcom;

// What a counting pass does, on the host: per group and digit value, the elements whose higher bits equal the group's prefix.
template <typename T>
static std::vector<uint64_t> count_pass(const std::vector<T> &v, const std::vector<uint64_t> &groups, int keybits, int pass)
{
    int shift, nbits;
    om_digit(keybits, pass, &shift, &nbits);
    std::vector<uint64_t> hist(groups.size() * OM_BINS, 0);
    for (T x : v) {
        if (x != x) continue;
        const uint64_t key = om_key(x);
        const int g = qt_find(groups.data(), (int)groups.size(), qt_high(key, shift + nbits));
        if (g >= 0) hist[(size_t)g * OM_BINS + ((key >> shift) & ((1u << nbits) - 1u))]++;
    }
    return hist;
}

template <typename T>
static bool same(T a, T b)
{
    return (a != a && b != b) || a == b;  // (-0.0 == 0.0: one value)
}

template <typename T>
static void check_select(const char *type, long *maxgroups)
{
    const int keybits = 8 * (int)sizeof(T);
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> normal;
    long checks = 0, fails = 0;
    for (int kind = 0; kind < 6; kind++)
        for (size_t n : {1u, 2u, 3u, 64u, 1000u, 20011u}) {
            std::vector<T> v(n);
            for (size_t i = 0; i < n; i++) {
                const double g = normal(rng);
                v[i] = kind == 0   ? (T)g
                       : kind == 1 ? (T)(std::round(g * 2) / 4)                                      // long ties
                       : kind == 2 ? (T)(g * std::pow(10.0, (double)((long)(rng() % 61) - 30)))       // many first digits
                       : kind == 3 ? (i % 7 == 0 ? std::numeric_limits<T>::quiet_NaN() : (T)g)       // NaNs sort last
                       : kind == 4 ? (i % 3 == 0 ? (T)0.0 : i % 3 == 1 ? (T)-0.0 : (T)g)
                                   : (i % 5 == 0 ? std::numeric_limits<T>::infinity() : i % 5 == 1 ? -std::numeric_limits<T>::infinity() : (T)(g * std::numeric_limits<T>::denorm_min() * 8));
            }
            std::vector<T> sorted;
            for (T x : v)
                if (x == x) sorted.push_back(x);
            std::sort(sorted.begin(), sorted.end());
            const size_t real = sorted.size();
            std::vector<size_t> want;  // 26 ranks: both ends, pairs of neighbours, repeats
            for (int r = 0; r < 13; r++) {
                const size_t k = (size_t)((double)(n - 1) * r / 12.0);
                want.push_back(k);
                want.push_back(std::min(k + 1, n - 1));
            }
            std::vector<QtRank> ranks(want.size());
            for (size_t r = 0; r < want.size(); r++) {
                ranks[r].live = want[r] < real;
                ranks[r].rank = ranks[r].live ? want[r] : 0;
            }
            for (int pass = 0; pass < om_passes(keybits); pass++) {
                int shift, nbits;
                om_digit(keybits, pass, &shift, &nbits);
                const std::vector<uint64_t> groups = qt_groups(ranks.data(), (int)ranks.size(), shift + nbits);
                *maxgroups = std::max(*maxgroups, (long)groups.size());
                for (size_t g = 1; g < groups.size(); g++) fails += !(groups[g - 1] < groups[g]);
                const std::vector<uint64_t> hist = count_pass(v, groups, keybits, pass);
                qt_advance(ranks.data(), (int)ranks.size(), groups, hist.data(), keybits, pass);
            }
            for (size_t r = 0; r < want.size(); r++) {
                checks++;
                if (!ranks[r].live) {
                    fails += want[r] < real;
                    continue;
                }
                const T got = sizeof(T) == 4 ? (T)om_value_f32(ranks[r].prefix) : (T)om_value_f64(ranks[r].prefix);
                fails += !same(got, sorted[want[r]]);
            }
        }
    printf("select %s %ld %ld\n", type, checks, fails);
    if (fails) exit(1);
}

// Positions on a grid of 1/8: every square and the sum are exact, so floor(sqrt(r2)) = j <=> j^2 <= r2 < (j + 1)^2 in integers (x 64).
static void check_rings()
{
    long checks = 0, fails = 0;
    const int n = 40, rpix = 9;
    for (int xi = -8 * 14; xi <= 8 * (n + 14); xi += 3)
        for (int yi = -8 * 3; yi <= 8 * (n + 3); yi += 37) {
            const double x = xi / 8.0, y = yi / 8.0;
            int x0, x1, y0, y1;
            qt_ring_box(x, rpix, n, &x0, &x1);
            qt_ring_box(y, rpix, n, &y0, &y1);
            const long fx = (xi >= 0 ? xi / 8 : -((-xi + 7) / 8)), cx = (xi >= 0 ? (xi + 7) / 8 : -((-xi) / 8));
            const long wx0 = std::min<long>(std::max<long>(fx - rpix - 1, 0), n), wx1 = std::min<long>(std::max<long>(cx + rpix + 1, 0), n);
            checks++;
            fails += !(x0 == wx0 && x1 == wx1 && y0 >= 0 && y1 <= n && y0 <= y1);
            for (int row = 0; row < n; row++)
                for (int col = 0; col < n; col++) {
                    const long dx = 8L * col - xi, dy = 8L * row - yi, r2 = dx * dx + dy * dy;  // x 64
                    long j = 0;
                    while (64 * (j + 1) * (j + 1) <= r2) j++;
                    checks++;
                    fails += qt_ring_index(col, row, x, y) != j;
                    // every pixel of a ring below rpix lies in the box
                    if (j < rpix) fails += !(col >= x0 && col < x1 && row >= y0 && row < y1);
                }
        }
    printf("rings float64 %ld %ld\n", checks, fails);
    if (fails) exit(1);
}

int main()
{
    long maxgroups = 0;
    check_select<float>("float32", &maxgroups);
    check_select<double>("float64", &maxgroups);
    printf("groups most %ld %d\n", maxgroups, maxgroups < 13 ? 1 : 0);  // (the many-first-digits arrays spread the ranks over many groups)
    check_rings();
    return maxgroups < 13;
}
