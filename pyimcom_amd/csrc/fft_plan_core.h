// fft_plan_core.h -- the plan of the wave-per-line FFT (fft_lines.h): which radices, where each stage's twiddle table starts, how many
// lines a workgroup holds and what that costs in LDS.  Plain host arithmetic with one right answer; compiles without HIP
// (tests/native/fft_plan_check.cpp).  Nothing outside this header writes a field of FftPlan.
#pragma once
#include <cstddef>

namespace imcom {

constexpr int WF_MAXN = 1024, WF_MAXST = 8;  // longest line, most stages
constexpr int WF_MAXWAVES = 12;  // waves per workgroup: three per SIMD leave a wave 168 registers (a radix-16 butterfly with its twiddles needs ~140)

struct FftPlan {
    int n, npad, nst, radix[WF_MAXST], twoff[WF_MAXST], twn, waves;  // npad: n rounded up to 16; waves per workgroup
};

// stage s > 0 (Ns = product of the earlier radices) owns (radix[s] - 1) Ns table values from twoff[s] on; stage 0 has no twiddles
inline void fft_plan_tables(FftPlan *pl)
{
    int Ns = pl->radix[0], off = 0;
    pl->twoff[0] = 0;
    for (int s = 1; s < pl->nst; s++) {
        pl->twoff[s] = off;
        off += (pl->radix[s] - 1) * Ns;
        Ns *= pl->radix[s];
    }
    pl->twn = off;
}

// n = product of radices 16, 8, 4, 2, 3, 5 (at least two stages) with lines that fit the wave engine?
inline bool fft_line_plan(int n, FftPlan *pl)
{
    if (n > WF_MAXN || n < 6) return false;
    pl->n = n;
    pl->npad = (n + 15) / 16 * 16;
    pl->nst = 0;
    int r = n;
    const int cand[6] = {16, 8, 4, 2, 3, 5};
    for (int ci = 0; ci < 6; ci++)
        while (r % cand[ci] == 0) {
            if (pl->nst >= WF_MAXST) return false;
            pl->radix[pl->nst++] = cand[ci];
            r /= cand[ci];
        }
    if (r != 1 || pl->nst < 2) return false;
    fft_plan_tables(pl);
    // as many waves (= lines) per workgroup as LDS holds next to the tables, WF_MAXWAVES at most
    const long line = (long)pl->npad * 16, lds = 160 * 1024, fit = (lds - (long)pl->twn * 16) / line;
    pl->waves = (int)(fit < WF_MAXWAVES ? fit : WF_MAXWAVES);
    return pl->waves >= 1;
}

// the sides 4, 8, 16, which fft_line_plan factors into one stage and refuses, as two stages -- for a caller that runs one such
// transform per wave on slices it lays out itself (noisespec.hip's sub-transforms)
inline bool fft_short_plan(int n, FftPlan *pl)
{
    if (n != 4 && n != 8 && n != 16) return false;
    pl->n = n, pl->npad = 16, pl->nst = 2, pl->waves = 1;
    pl->radix[0] = n == 4 ? 2 : 4, pl->radix[1] = n / pl->radix[0];
    fft_plan_tables(pl);
    return true;
}

// dynamic LDS of a line kernel: `slices` line slices of npad values, the stage tables behind them
inline size_t fft_line_lds_bytes(const FftPlan &pl, int slices) { return ((size_t)slices * pl.npad + pl.twn) * 16; }
inline size_t fft_line_lds_bytes(const FftPlan &pl) { return fft_line_lds_bytes(pl, pl.waves); }

}  // namespace imcom
