// poisson_core.h -- numpy's Poisson draw (random_poisson of numpy/random/src/distributions/distributions.c) restated by stream position,
// without a device in it.  Compiles as host code too (tests/native/poisson_check.cpp).
//
// Generator.poisson(lam = array) calls random_poisson(lam_i) per element in C order.  Every uniform it takes is next_double = (out >> 11)
// 2^-53 of one 64-bit output, so a draw that starts at stream position p reads U[p], U[p + 1], ...:
//   lam == 0       returns 0 and reads nothing.
//   0 < lam < 10   (random_poisson_mult) enlam = exp(-lam), prod = 1; prod *= U and X counts up while prod > enlam: X + 1 outputs.
//   lam >= 10      (random_poisson_ptrs, Hoermann's transformed rejection) attempts of two outputs, U = next - 0.5 and V = next, with
//                  us = 0.5 - |U| and k = floor((2 a / us + b) U + lam + 0.43): accepted at once if us >= 0.07 && V <= vr (69 % at lam =
//                  86), refused if k < 0 || (us < 0.013 && V > us), and else accepted iff
//                      log(V) + log(invalpha) - log(a / us^2 + b)  <=  -lam + k log(lam) - loggam(k + 1)            (the slow test)
//                  with numpy's own ten-term series for loggam.
// All arithmetic is IEEE double in numpy's order with contraction off (the pragma below: this header turns contraction off for the rest
// of the translation unit that includes it), sqrt and division correctly rounded: given the same U, two machines differ only in what
// their libm returns for log and exp.
//
// The guard band.  Every basic operation is the same on both sides, so two evaluations of a comparison differ by what the log / exp
// results differ (each within 1 ulp of the truth, so at most 2 ulp = 4 u of each other, u = 2^-53) and by the roundings of the operations
// that take those results in (at most 1 ulp = 2 u of the intermediate each, beyond the difference they carry).
//   The slow test is a difference of sums whose terms reach 1e6 in a star's core (k log(lam), loggam(k + 1)) and cancel, so its band is
//   ABSOLUTE: guard * M, M the sum of the magnitudes of every term on both sides: |log V|, |log invalpha|, |log(a / us^2 + b)|, lam,
//   |k log lam|, and inside loggam |gl0 / x0|, 0.5 lg2pi, |(x0 - 0.5) log x0|, x0 and each |log(x0 - 1)| of the recurrence.  The logs give
//   4 u M, the two products that take a log in 2 * 2 u M, and the 13 additions at most (2 on the left, 2 on the right, 3 + 6 in loggam)
//   2 u M each: 34 u M in all.  POI_GUARD = 64 u = 2^-47 is nearly twice that.
//   prod > enlam: prod is made of exact uniforms and roundings alone; enlam = exp(-lam) differs by at most 4 u enlam.  Its band is
//   relative, guard * enlam (16 times what is needed).
// A comparison inside its band still takes numpy's branch as this libm sees it, and flags the draw POI_UNDECIDED; a caller that finds
// the flag on a draw of the path has the whole request drawn by numpy.
//   How often, at bg = 86 (k near 86): M = lam + k log lam + (k + .5) log(k + 1) + k + ... = 86 + 383 + 386 + 87 + 6 = 950, so the band is
//   2 * 64 u * 950 = 1.35e-11 wide.  The left side holds log V with V uniform, whose density in log V is V <= 1, so a slow test lands in
//   the band with probability at most 1.35e-11.  Measured with this code, a draw at lam = 86 makes 0.37 slow tests (1.178 attempts, 69 %
//   of them accepted at once): 6.2e6 per 4088^2 frame, so at most 8.4e-5 of the frames are undecided, one in 1.2e4; with the density of
//   log V where slow tests happen (V about 0.5) one in 2.4e4.  A star's core adds little: M = 1e6 there widens the band 1000 times for
//   the few hundred pixels that have it.
// Loop caps.  A PTRS draw may take POI_PTRS_CAP = 32 attempts: the refusal rate is highest at lam = 10 (0.25 per attempt; 0.15 at 86), so
// a draw reaches the cap with probability below 0.25^32 = 5e-20, 1e-12 per frame of 1.7e7 draws.  A mult draw may take POI_MULT_CAP = 64
// outputs: X >= 64 at lam < 10 has probability below 1e-28.  A draw at its cap is POI_OVERCAP, which callers treat as undecided.
// No draw reads more than POI_HALO = 64 outputs.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define POI_HD __host__ __device__ __forceinline__
#else
#define POI_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace imcom {

constexpr int POI_PTRS_CAP = 32, POI_MULT_CAP = 64, POI_HALO = 64;
constexpr double POI_GUARD = 0x1.0p-47;
constexpr double POI_LAM_MAX = 9.223372006484771e+18;  // numpy's POISSON_LAM_MAX: int64 max - 10 sqrt(int64 max)
enum { POI_ZERO = 0, POI_MULT = 1, POI_PTRS = 2 };
enum { POI_UNDECIDED = 1, POI_OVERCAP = 2 };

struct PoiDraw {
    long value;
    int adv;     // outputs consumed, 0 .. POI_HALO
    int flags;   // POI_UNDECIDED | POI_OVERCAP
    int branch;  // POI_ZERO / POI_MULT / POI_PTRS
    int slow;    // slow tests made
};

POI_HD double poi_uniform(uint64_t w) { return (double)(w >> 11) * 0x1.0p-53; }
POI_HD bool poi_lam_valid(double lam) { return lam >= 0.0 && lam <= POI_LAM_MAX; }  // (a NaN compares false)
// the least a draw of this rate consumes
POI_HD int poi_min_adv(double lam) { return !(lam > 0.0) ? 0 : (lam < 10.0 ? 1 : 2); }

// numpy's random_loggam; *mag takes the magnitudes of its terms
POI_HD double poi_loggam(double x, double *mag)
{
    const double a[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
                          -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00};
    if (x == 1.0 || x == 2.0) return 0.0;
    const int n = x < 7.0 ? (int)(7 - x) : 0;
    double x0 = x + n;
    const double x2 = (1.0 / x0) * (1.0 / x0), lg2pi = 1.8378770664093453e+00;
    double gl0 = a[9];
    for (int k = 8; k >= 0; k--) {
        gl0 *= x2;
        gl0 += a[k];
    }
    const double t0 = gl0 / x0, t1 = 0.5 * lg2pi, t2 = (x0 - 0.5) * log(x0);
    double gl = t0 + t1 + t2 - x0;
    *mag += fabs(t0) + t1 + fabs(t2) + x0;
    if (x < 7.0)
        for (int k = 1; k <= n; k++) {
            const double l = log(x0 - 1.0);
            gl -= l;
            *mag += fabs(l);
            x0 -= 1.0;
        }
    return gl;
}

// One attempt of random_poisson_ptrs, in two steps so that a kernel can take the slow tests of many attempts together.
struct PoiPtrs {  // the constants of a rate
    double loglam, b, a, invalpha, vr;
};
POI_HD PoiPtrs poi_ptrs_consts(double lam)
{
    PoiPtrs c;
    const double slam = sqrt(lam);
    c.loglam = log(lam);
    c.b = 0.931 + 2.53 * slam;
    c.a = -0.059 + 0.02483 * c.b;
    c.invalpha = 1.1239 + 1.1328 / (c.b - 3.4);
    c.vr = 0.9277 - 3.6224 / (c.b - 2);
    return c;
}
enum { POI_ACCEPT = 0, POI_REJECT = 1, POI_SLOW = 2 };
// the two quick tests of the attempt that reads raw[0], raw[1]: POI_ACCEPT (*kf is the value), POI_REJECT, or POI_SLOW: poi_ptrs_slow decides
POI_HD int poi_ptrs_quick(const PoiPtrs &c, double lam, const uint64_t *raw, double *kf)
{
    const double U = poi_uniform(raw[0]) - 0.5, V = poi_uniform(raw[1]);
    const double us = 0.5 - fabs(U);
    *kf = floor((2 * c.a / us + c.b) * U + lam + 0.43);
    if (us >= 0.07 && V <= c.vr) return POI_ACCEPT;
    if (*kf < 0 || (us < 0.013 && V > us)) return POI_REJECT;
    return POI_SLOW;
}
// the slow test of the same attempt: POI_ACCEPT or POI_REJECT; *flags takes POI_UNDECIDED
POI_HD int poi_ptrs_slow(const PoiPtrs &c, double lam, const uint64_t *raw, double guard, double *kf, int *flags)
{
    const double U = poi_uniform(raw[0]) - 0.5, V = poi_uniform(raw[1]);
    const double us = 0.5 - fabs(U);
    *kf = floor((2 * c.a / us + c.b) * U + lam + 0.43);
    if (!(*kf < 9.2e18)) {  // us == 0 and V == 0 (2^-106): numpy's conversion of an infinite k is not defined
        *flags |= POI_UNDECIDED;
        *kf = 0.0;
        return POI_ACCEPT;
    }
    const double l0 = log(V), l1 = log(c.invalpha), l2 = log(c.a / (us * us) + c.b), kl = *kf * c.loglam;
    double mag = fabs(l0) + fabs(l1) + fabs(l2) + lam + fabs(kl);
    const double lg = poi_loggam((double)((long)*kf + 1), &mag);
    const double lhs = l0 + l1 - l2, rhs = -lam + kl - lg;
    if (!(fabs(lhs - rhs) > guard * mag)) *flags |= POI_UNDECIDED;  // (also V == 0: both infinite)
    return lhs <= rhs ? POI_ACCEPT : POI_REJECT;
}

// The draw of rate lam (valid, see poi_lam_valid) whose first output is raw[0]; raw[1 .. POI_HALO - 1] are readable.
POI_HD PoiDraw poi_draw(double lam, const uint64_t *raw, double guard)
{
    PoiDraw d = {0, 0, 0, POI_ZERO, 0};
    if (!(lam > 0.0)) return d;
    if (lam < 10.0) {
        d.branch = POI_MULT;
        const double enlam = exp(-lam);
        double prod = 1.0;
        for (int t = 0; t < POI_MULT_CAP; t++) {
            prod *= poi_uniform(raw[t]);
            d.adv = t + 1;
            if (fabs(prod - enlam) <= guard * enlam) d.flags |= POI_UNDECIDED;
            if (!(prod > enlam)) return d;
            d.value++;
        }
        d.flags |= POI_OVERCAP;
        return d;
    }
    d.branch = POI_PTRS;
    const PoiPtrs c = poi_ptrs_consts(lam);
    for (int t = 0; t < POI_PTRS_CAP; t++) {
        double kf;
        int r = poi_ptrs_quick(c, lam, raw + 2 * t, &kf);
        d.adv = 2 * t + 2;
        if (r == POI_SLOW) {
            d.slow++;
            r = poi_ptrs_slow(c, lam, raw + 2 * t, guard, &kf, &d.flags);
        }
        if (r == POI_ACCEPT) {
            d.value = (long)kf;
            return d;
        }
    }
    d.flags |= POI_OVERCAP;
    return d;
}

// ---- the window scheme shared by poisson.hip and its host mirror below -----------------------------------------------------------------
// Draws are taken in superchunks of S; positions count from the superchunk's entry.  With m_j = poi_min_adv and mb_j its exclusive
// prefix sum, draw j at position p has the excess x = p - mb_j >= 0, which never decreases along the path.  Layer j's window is the W
// excesses from lo_j = max(0, (D_j >> 8) - W / 2), D_j the exclusive prefix sum of poi_drift256: the expected gain of excess of a draw in
// 1/256 outputs (lam for a mult draw; two outputs per refused PTRS attempt, measured and interpolated in 1 / sqrt(lam)).  The window only
// decides which superchunks are redone by the sequential walk; no result depends on it.  A PTRS node is resolved attempt by attempt inside
// its layer's window (a refused attempt at excess x continues at x + 2), so it also leaves the window when one of its attempts would
// start at or beyond lo_j + W, or after POI_PTRS_CAP - 1 refusals (poi_node_leaves).
constexpr int POI_X_BITS = 28, POI_X_MASK = (1 << POI_X_BITS) - 1, POI_LEAVE = -1;  // a node: next excess | flags << 28, or POI_LEAVE

POI_HD int poi_drift256(double lam)
{
    if (!(lam > 0.0)) return 0;
    if (lam < 10.0) return (int)(lam * 256.0);
    // outputs beyond two per PTRS draw at 1 / sqrt(lam) = 0, 0.04, .. 0.32, measured with poi_draw over 4e6 draws each (0.3561 at lam = 86,
    // where this gives 0.3562; the standard deviation per draw is 0.75 to 1.32)
    const double tab[9] = {0.2480, 0.2853, 0.3260, 0.3702, 0.4181, 0.4708, 0.5288, 0.5934, 0.6646};
    const double x = 25.0 / sqrt(lam);
    const int i = x >= 7.0 ? 7 : (int)x;
    return (int)(256.0 * (tab[i] + (tab[i + 1] - tab[i]) * (x - i)) + 0.5);
}
// slot w of a layer's window, a draw that consumed adv outputs
POI_HD bool poi_node_leaves(int branch, int w, int adv, int W) { return branch == POI_PTRS && (w + adv - 2 >= W || adv >= 2 * POI_PTRS_CAP); }
POI_HD int poi_window_lo(long D, int W)
{
    const long lo = (D >> 8) - W / 2;
    return lo > 0 ? (int)lo : 0;
}

}  // namespace imcom

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host: the scheme of poisson.hip, step for step ------------------------------------------------------------------------------------
#include <algorithm>
#include <vector>

namespace imcom {

struct PoiDraws {
    std::vector<long> out;
    std::vector<int> adv;      // outputs each draw consumed
    uint64_t consumed = 0;
    long recovered = 0;        // superchunks whose path left a window and that the walk redid
    long offpath_flags = 0;    // window nodes off the path that were undecided or over a cap
    bool undecided = false, short_of_outputs = false;
};

// `count` draws of the rates lam[] from the outputs raw[0 .. nraw): superchunks of S draws, windows of W excesses, tiles of T layers
// (S a multiple of T); force_walk: every superchunk by the sequential walk
inline PoiDraws poi_draws(const uint64_t *raw_in, long nraw, const double *lam, long count, int S, int W, int T, double guard, bool force_walk)
{
    PoiDraws r;
    r.out.assign((size_t)count, 0);
    r.adv.assign((size_t)count, 0);
    std::vector<uint64_t> raw((size_t)nraw + POI_HALO, 0);
    for (long i = 0; i < nraw; i++) raw[(size_t)i] = raw_in[i];
    uint64_t p0 = 0;
    for (long s0 = 0; s0 < count; s0 += S) {
        const int ns = (int)std::min<long>(S, count - s0), ntile = (ns + T - 1) / T;
        std::vector<int> mb((size_t)ns + 1, 0);
        std::vector<long> D((size_t)ns + 1, 0);
        for (int j = 0; j < ns; j++) {
            mb[j + 1] = mb[j] + poi_min_adv(lam[s0 + j]);
            D[j + 1] = D[j] + poi_drift256(lam[s0 + j]);
        }
        const long need = (long)mb[ns] + poi_window_lo(D[ns], W) + W + POI_HALO;
        if (p0 + (uint64_t)need > (uint64_t)nraw + POI_HALO) {
            r.short_of_outputs = true;
            return r;
        }
        const uint64_t *u = raw.data() + p0;
        bool recover = force_walk;
        std::vector<int> entry((size_t)ntile, 0);
        int e = 0, pathflags = 0;
        if (!force_walk) {
            // node table and tile maps: every entry slot of a tile walks its T layers through the windows
            std::vector<int> tilemap((size_t)ntile * W);
            for (int t = 0; t < ntile; t++) {
                const int j0 = t * T, j1 = std::min(ns, j0 + T);
                std::vector<int> cur((size_t)W), row((size_t)W);
                for (int w = 0; w < W; w++) cur[w] = poi_window_lo(D[j0], W) + w;
                for (int j = j0; j < j1; j++) {
                    const int lo = poi_window_lo(D[j], W), m = poi_min_adv(lam[s0 + j]);
                    for (int w = 0; w < W; w++) {
                        const PoiDraw d = poi_draw(lam[s0 + j], u + mb[j] + lo + w, guard);
                        row[w] = poi_node_leaves(d.branch, w, d.adv, W) ? POI_LEAVE : (lo + w + d.adv - m) | (d.flags << POI_X_BITS);
                    }
                    for (int w = 0; w < W; w++) {
                        if (cur[w] < 0) continue;
                        const int idx = (cur[w] & POI_X_MASK) - lo;
                        cur[w] = idx < 0 || idx >= W || row[idx] < 0 ? POI_LEAVE : ((row[idx] & POI_X_MASK) | ((cur[w] | row[idx]) & ~POI_X_MASK));
                    }
                }
                for (int w = 0; w < W; w++) tilemap[(size_t)t * W + w] = cur[w];
            }
            // chain: the tile entries from the true entry, excess 0
            for (int t = 0; t < ntile && !recover; t++) {
                const int idx = e - poi_window_lo(D[t * T], W);
                const int v = idx < 0 || idx >= W ? POI_LEAVE : tilemap[(size_t)t * W + idx];
                entry[t] = e;
                if (v < 0) {
                    recover = true;
                    break;
                }
                e = v & POI_X_MASK;
                pathflags |= v >> POI_X_BITS;
            }
            if (recover) r.recovered++;
        }
        if (!recover) {
            // values: every tile from its entry
            int on_path = 0;
            for (int t = 0; t < ntile; t++) {
                int x = entry[t];
                for (int j = t * T; j < std::min(ns, t * T + T); j++) {
                    const PoiDraw d = poi_draw(lam[s0 + j], u + mb[j] + x, guard);
                    r.out[s0 + j] = d.value;
                    r.adv[s0 + j] = d.adv;
                    on_path |= d.flags;
                    x += d.adv - poi_min_adv(lam[s0 + j]);
                }
            }
            if (on_path != pathflags) r.short_of_outputs = true;  // (the maps and the walk of the path disagree: never)
            if (on_path) r.undecided = true;
            p0 += (uint64_t)(mb[ns] + e);
        } else {
            uint64_t p = p0;
            for (int j = 0; j < ns; j++) {
                if (p + POI_HALO > (uint64_t)nraw + POI_HALO) {
                    r.short_of_outputs = true;
                    return r;
                }
                const PoiDraw d = poi_draw(lam[s0 + j], raw.data() + p, guard);
                r.out[s0 + j] = d.value;
                r.adv[s0 + j] = d.adv;
                if (d.flags) r.undecided = true;
                p += (uint64_t)d.adv;
            }
            p0 = p;
        }
    }
    r.consumed = p0;
    if (r.consumed > (uint64_t)nraw) r.short_of_outputs = true;
    return r;
}

}  // namespace imcom
#endif
