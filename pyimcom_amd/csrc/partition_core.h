// partition_core.h -- the visiting order of InImage.partition_pixels (reference src/pyimcom/coadd.py:331-341) as arithmetic on a visit
// index: the relevant sparse-grid cells row-major, the pixels row-major inside a cell; cell (j, i) spans the columns sp_arr[i] .. sp_arr[i + 1]
// and the rows sp_arr[j] .. sp_arr[j + 1].  The cells are NOT of one size (np.linspace(..., dtype=np.uint16) truncates), so the index is
// decoded from a prefix sum over the relevant cells.  Compiles as host code too (tests/native/partition_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PART_HD __host__ __device__ __forceinline__
#else
#define PART_HD inline
#endif

namespace imcom {

// The relevant cells that hold a pixel, in visiting order: start[c] = visit index of the first pixel of cell c (start[ncell] = all visits),
// cell[c] = j * sp_res + i.  Returns ncell; `start` has room for sp_res^2 + 1 entries and `cell` for sp_res^2.  Host side.
inline int partition_cells(const unsigned short *sp_arr, const unsigned char *relevant, int sp_res, unsigned int *start, unsigned int *cell)
{
    int nc = 0;
    uint64_t run = 0;
    for (int j = 0; j < sp_res; j++)
        for (int i = 0; i < sp_res; i++) {
            if (!relevant[j * sp_res + i]) continue;
            const uint64_t h = sp_arr[j + 1] > sp_arr[j] ? sp_arr[j + 1] - sp_arr[j] : 0, w = sp_arr[i + 1] > sp_arr[i] ? sp_arr[i + 1] - sp_arr[i] : 0;
            if (h * w == 0) continue;  // (an empty cell is visited by nobody and would break the search below)
            start[nc] = (unsigned int)run;
            cell[nc++] = (unsigned int)(j * sp_res + i);
            run += h * w;  // (at most 65535^2 < 2^32: the axis is uint16 and nondecreasing)
        }
    start[nc] = (unsigned int)run;
    return nc;
}

// Visit index p (< start[ncell]) -> the pixel (y, x) of the input image.  start is strictly increasing over 0 .. ncell.
PART_HD void partition_decode(const unsigned int *start, const unsigned int *cell, int ncell, const unsigned short *sp_arr, int sp_res, unsigned int p, int *y,
                              int *x)
{
    int lo = 0, hi = ncell - 1;  // the last c with start[c] <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    const unsigned int c = cell[lo], j = c / (unsigned int)sp_res, i = c - j * (unsigned int)sp_res;
    const unsigned int left = sp_arr[i], w = sp_arr[i + 1] - left, r = p - start[lo], row = r / w;
    *y = (int)(sp_arr[j] + row);
    *x = (int)(left + (r - row * w));
}

}  // namespace imcom
