// objmask_check.cpp -- the host-compilable core of csrc/objmask.hip (objmask_core.h): the order-preserving keys and the digit walk of the
// radix select against std::nth_element, and the row step of the constrained flood, run to a tile's fixpoint, against a queue flood
// fill.  Prints one line per check; a non-zero exit on the first difference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <deque>
#include <limits>
#include <random>
#include <vector>

#include "objmask_core.h"

using namespace imcom;

// the selection of objmask.hip, serially: per pass a histogram of the digit among the keys whose higher digits match the prefix
template <typename T>
static T radix_select(const std::vector<T> &v, size_t rank)
{
    const int keybits = 8 * (int)sizeof(T);
    uint64_t prefix = 0;
    for (int pass = 0; pass < om_passes(keybits); pass++) {
        int shift, nbits;
        om_digit(keybits, pass, &shift, &nbits);
        const int top = shift + nbits;
        std::vector<size_t> h((size_t)1 << nbits, 0);
        for (T x : v) {
            const uint64_t key = om_key(x);
            if ((top >= 64 ? 0 : key >> top) == (top >= 64 ? 0 : prefix >> top)) h[(key >> shift) & (((uint64_t)1 << nbits) - 1)]++;
        }
        size_t cum = 0, d = 0;
        while (d + 1 < h.size() && cum + h[d] <= rank) cum += h[d++];
        rank -= cum;
        prefix |= (uint64_t)d << shift;
    }
    if (sizeof(T) == 4) return (T)om_value_f32(prefix);
    return (T)om_value_f64(prefix);
}

template <typename T>
static int check_select(const char *name)
{
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> gauss(0.0, 3.0);
    const T inf = std::numeric_limits<T>::infinity();
    int bad = 0, cases = 0;
    for (size_t n : {1u, 2u, 3u, 255u, 256u, 257u, 5000u}) {
        for (int kind = 0; kind < 4; kind++) {
            std::vector<T> v(n);
            for (size_t i = 0; i < n; i++) {
                const double g = gauss(rng);
                v[i] = kind == 0 ? (T)g : kind == 1 ? (T)std::floor(g) : kind == 2 ? std::nextafter((T)1, (T)(1 + (int)(rng() % 5))) : (T)(g * 1e30);
            }
            if (kind == 1 && n > 2) v[0] = (T)-0.0, v[1] = (T)0.0, v[2] = -inf;
            if (kind == 3 && n > 2) v[0] = inf, v[1] = -inf, v[2] = std::numeric_limits<T>::denorm_min();
            for (size_t rank : {(size_t)0, (n - 1) / 2, n / 2, n - 1}) {
                std::vector<T> w(v);
                std::nth_element(w.begin(), w.begin() + rank, w.end());
                cases++;
                if (!(radix_select(v, rank) == w[rank])) bad++;  // (== : -0.0 and 0.0 are one value)
            }
        }
    }
    // keys keep the order of neighbouring values through zero and to the infinities
    const T probe[] = {-inf, (T)-1e30, (T)-1, -std::numeric_limits<T>::denorm_min(), (T)0, std::numeric_limits<T>::denorm_min(), (T)1, (T)1e30, inf};
    for (size_t i = 0; i + 1 < sizeof(probe) / sizeof(probe[0]); i++)
        if (!(om_key(probe[i]) < om_key(probe[i + 1]))) bad++;
    if (om_key((T)-0.0) != om_key((T)0.0)) bad++;
    printf("select %s %d %d\n", name, cases, bad);
    return bad;
}

static int check_flood()
{
    std::mt19937_64 rng(777);
    int bad = 0, cases = 0;
    for (int trial = 0; trial < 40; trial++) {
        uint64_t g[64], s[64], want[64];
        const unsigned density = 2 + trial % 3;  // grow bits: AND of fewer words is denser
        for (int j = 0; j < 64; j++) {
            g[j] = rng() | rng();
            for (unsigned q = 0; q < density; q++) g[j] &= rng() | rng();
            s[j] = (rng() & rng() & rng() & rng() & rng());  // a few seeds, in and out of grow
            want[j] = s[j];
        }
        std::deque<std::pair<int, int>> queue;
        for (int j = 0; j < 64; j++)
            for (int c = 0; c < 64; c++)
                if ((s[j] >> c) & 1) queue.push_back({j, c});
        while (!queue.empty()) {
            auto [j, c] = queue.front();
            queue.pop_front();
            const int dj[4] = {-1, 1, 0, 0}, dc[4] = {0, 0, -1, 1};
            for (int q = 0; q < 4; q++) {
                const int y = j + dj[q], x = c + dc[q];
                if (y < 0 || y > 63 || x < 0 || x > 63 || !((g[y] >> x) & 1) || ((want[y] >> x) & 1)) continue;
                want[y] |= (uint64_t)1 << x;
                queue.push_back({y, x});
            }
        }
        int rounds = 0;
        for (bool moved = true; moved && rounds <= 64 * 64; rounds++) {  // the kernel's loop: all rows step from the same state
            uint64_t n[64];
            moved = false;
            for (int j = 0; j < 64; j++) n[j] = om_flood_row(s[j], j ? s[j - 1] : 0, j < 63 ? s[j + 1] : 0, g[j]);
            for (int j = 0; j < 64; j++) moved |= n[j] != s[j], s[j] = n[j];
        }
        cases++;
        for (int j = 0; j < 64; j++)
            if (s[j] != want[j]) { bad++; break; }
        if (rounds > 64 * 64) bad++;
    }
    printf("flood tile %d %d\n", cases, bad);
    return bad;
}

int main()
{
    int bad = check_select<float>("float32");
    bad += check_select<double>("float64");
    bad += check_flood();
    return bad ? 1 : 0;
}
