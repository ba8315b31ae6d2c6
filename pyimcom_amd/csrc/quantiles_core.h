// quantiles_core.h -- the arithmetic of quantiles.hip that has one right answer and no device in it: the walk of a digit's histogram to the
// bin that holds a rank, the grouping of many ranks by the key prefix they have reached, the search of a key's prefix among a segment's
// live groups, and the ring a pixel belongs to around a star.  The keys and the digit schedule are objmask_core.h's.  Compiles as host
// code too (tests/native/quantiles_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "objmask_core.h"

namespace imcom {

// The bits of a key above the digit of `pass` (0 in the first pass: one group holds every key).
OM_HD uint64_t qt_high(uint64_t key, int top) { return top >= 64 ? 0ull : key >> top; }

// Index of `hi` among the n ascending values of `sorted`, or -1.
OM_HD int qt_find(const uint64_t *sorted, int n, uint64_t hi)
{
    int lo = 0, up = n;
    while (lo < up) {
        const int mid = (lo + up) >> 1;
        if (sorted[mid] < hi) lo = mid + 1;
        else up = mid;
    }
    return (lo < n && sorted[lo] == hi) ? lo : -1;
}

// The clipped box of a star along one axis: clip(int16(floor(p)) - rpix - 1, 0, n) .. clip(int16(ceil(p)) + rpix + 1, 0, n).  The caller
// has made sure that |p| + rpix + 1 < 32767 and n <= 32767, so the int16 arithmetic of the reference neither wraps nor differs from int.
OM_HD void qt_ring_box(double p, int rpix, int n, int *lo, int *hi)
{
    const int a = (int)floor(p) - rpix - 1, b = (int)ceil(p) + rpix + 1;
    *lo = a < 0 ? 0 : (a > n ? n : a);
    *hi = b < 0 ? 0 : (b > n ? n : b);
}

// floor(sqrt((col - x)^2 + (row - y)^2)) as numpy forms it in float64: two differences, two squares, one sum, each rounded once, the
// correctly rounded square root, the floor.  No fused multiply-add may form: contraction is switched off for this function and every
// step is a statement of its own.
OM_HD int qt_ring_index(int col, int row, double x, double y)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dx = (double)col - x;
    const double dy = (double)row - y;
    const double sx = dx * dx;
    const double sy = dy * dy;
    const double r2 = sx + sy;
#ifdef __HIP_DEVICE_COMPILE__
    return (int)floor(__dsqrt_rn(r2));
#else
    return (int)std::floor(std::sqrt(r2));
#endif
}

// ---- host functions: the selection's bookkeeping ---------------------------------------------------------------------------------------

// The bin of `hist` [bins] that holds rank `*rank` (0-based among the group's elements); *rank becomes the rank inside that bin.
inline int qt_walk(const uint64_t *hist, int bins, uint64_t *rank)
{
    uint64_t cum = 0;
    int d = 0;
    while (d < bins - 1 && cum + hist[d] <= *rank) cum += hist[d++];
    *rank -= cum;
    return d;
}

// One target rank of a segment on its way down the digits.
struct QtRank {
    uint64_t prefix = 0;  // the key's bits decided so far (in place, lower bits 0)
    uint64_t rank = 0;    // rank among the elements that share the prefix
    bool live = false;    // false: the answer is NaN (no such rank, a rank among the NaNs, an empty segment)
};

// The distinct values of qt_high(prefix, top) of the live ranks, ascending: the groups of the next pass.
inline std::vector<uint64_t> qt_groups(const QtRank *r, int n, int top)
{
    std::vector<uint64_t> g;
    for (int i = 0; i < n; i++)
        if (r[i].live) g.push_back(qt_high(r[i].prefix, top));
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());
    return g;
}

// One pass for one segment: `groups` as qt_groups gave them for this pass, hist [groups.size()][bins] what the pass counted.  Every live
// rank finds its digit and lengthens its prefix.
inline void qt_advance(QtRank *r, int n, const std::vector<uint64_t> &groups, const uint64_t *hist, int keybits, int pass)
{
    int shift, nbits;
    om_digit(keybits, pass, &shift, &nbits);
    const int top = shift + nbits, bins = 1 << nbits;
    for (int i = 0; i < n; i++) {
        if (!r[i].live) continue;
        const int g = qt_find(groups.data(), (int)groups.size(), qt_high(r[i].prefix, top));
        const int d = qt_walk(hist + (size_t)g * OM_BINS, bins, &r[i].rank);
        r[i].prefix |= (uint64_t)d << shift;
    }
}

}  // namespace imcom
