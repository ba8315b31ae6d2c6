// fft_plan_check.cpp -- csrc/fft_plan_core.h as a host program (built with -fsanitize=address,undefined by tests/test_fft_plan.py).
// Prints one line per side n = 2 .. 1024 of fft_line_plan, then one per side 4, 8, 16 of fft_short_plan:
//   "line n none"   or   "line n nst r0,r1,.. o0,o1,.. twn npad waves lds"      ("short n ..." likewise)
#include <cstdio>
#include <cstring>

#include "fft_plan_core.h"

using namespace imcom;

static void show(const char *kind, int n, bool ok, const FftPlan &pl)
{
    if (!ok) {
        printf("%s %d none\n", kind, n);
        return;
    }
    printf("%s %d %d ", kind, pl.n, pl.nst);
    for (int s = 0; s < pl.nst; s++) printf("%d%s", pl.radix[s], s + 1 < pl.nst ? "," : " ");
    for (int s = 0; s < pl.nst; s++) printf("%d%s", pl.twoff[s], s + 1 < pl.nst ? "," : " ");
    printf("%d %d %d %zu\n", pl.twn, pl.npad, pl.waves, fft_line_lds_bytes(pl));
}

int main()
{
    for (int n = 2; n <= WF_MAXN; n++) {
        FftPlan pl;
        memset(&pl, 0xff, sizeof pl);  // a field the planner forgot would show
        show("line", n, fft_line_plan(n, &pl), pl);
    }
    const int shorts[3] = {4, 8, 16};
    for (int n : shorts) {
        FftPlan pl;
        memset(&pl, 0xff, sizeof pl);
        show("short", n, fft_short_plan(n, &pl), pl);
    }
    FftPlan pl;
    return (fft_line_plan(WF_MAXN + 1, &pl) || fft_short_plan(32, &pl) || fft_short_plan(2, &pl)) ? 1 : 0;
}
