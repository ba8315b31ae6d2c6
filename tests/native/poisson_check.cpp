// poisson_check.cpp -- the host-compilable core of poisson.hip (csrc/poisson_core.h) against vectors of the Python restatement
// (tests/poisson_reference.py), as a stand-alone program for the sanitizers: tests/test_poisson_host.py builds it with
// -fsanitize=address,undefined, writes the vectors and runs it.
//
//   poisson_check FILE...   a file: int64 nraw, count, consumed; uint64 raw[nraw]; double lam[count]; int64 values[count]; int64 adv[count]
//
// Every file is drawn (1) one draw after another with poi_draw, (2) through the window tables and the recovery (poi_draws) for S in
// {4, 64}, W in {2, 8, 64}, T in {4, 16} (T = 16 only where S is a multiple of it) and by the forced walk, each with the production guard
// band and with none.  Values, the consumption of every draw and the total are compared.  One line a file: its name, the combinations run,
// the superchunks recovered over all of them, the draws of each branch.
#include <cstdio>
#include <cstring>
#include <vector>

#include "poisson_core.h"

using namespace imcom;

int main(int argc, char **argv)
{
    for (int f = 1; f < argc; f++) {
        FILE *fp = fopen(argv[f], "rb");
        if (!fp) return 2;
        long head[3];
        if (fread(head, 8, 3, fp) != 3) return 2;
        const long nraw = head[0], count = head[1], consumed = head[2];
        std::vector<uint64_t> raw((size_t)nraw);
        std::vector<double> lam((size_t)count);
        std::vector<long> want((size_t)count), adv((size_t)count);
        if (fread(raw.data(), 8, (size_t)nraw, fp) != (size_t)nraw || fread(lam.data(), 8, (size_t)count, fp) != (size_t)count ||
            fread(want.data(), 8, (size_t)count, fp) != (size_t)count || fread(adv.data(), 8, (size_t)count, fp) != (size_t)count)
            return 2;
        fclose(fp);
        long branch[3] = {0, 0, 0};
        {
            std::vector<uint64_t> padded(raw);
            padded.resize((size_t)nraw + POI_HALO, 0);
            long p = 0;
            for (long i = 0; i < count; i++) {
                if (!poi_lam_valid(lam[(size_t)i]) || p > nraw) return 2;
                const PoiDraw d = poi_draw(lam[(size_t)i], padded.data() + p, POI_GUARD);
                if (d.value != want[(size_t)i] || d.adv != adv[(size_t)i] || d.adv < poi_min_adv(lam[(size_t)i]) || d.flags) {
                    printf("%s: draw %ld (lam %a) is %ld after %d outputs (flags %d), expected %ld after %ld\n", argv[f], i, lam[(size_t)i], d.value, d.adv, d.flags,
                           want[(size_t)i], adv[(size_t)i]);
                    return 1;
                }
                branch[d.branch]++;
                p += d.adv;
            }
            if (p != consumed) {
                printf("%s: consumed %ld, expected %ld\n", argv[f], p, consumed);
                return 1;
            }
        }
        int combos = 0;
        long recovered = 0;
        const int Ss[2] = {4, 64}, Ws[3] = {2, 8, 64}, Ts[2] = {4, 16};
        for (int is = 0; is < 2; is++)
            for (int iw = 0; iw < 3; iw++)
                for (int it = 0; it < 2; it++)
                    for (int walk = 0; walk < 2; walk++)
                        for (int g = 0; g < 2; g++) {
                            const int S = Ss[is], W = Ws[iw], T = Ts[it];
                            if (S % T) continue;
                            const PoiDraws d = poi_draws(raw.data(), nraw, lam.data(), count, S, W, T, g ? POI_GUARD : 0.0, walk != 0);
                            if (d.undecided || d.short_of_outputs) {
                                printf("%s: S %d W %d T %d walk %d guard %d: undecided %d short %d\n", argv[f], S, W, T, walk, g, (int)d.undecided,
                                       (int)d.short_of_outputs);
                                return 1;
                            }
                            for (long i = 0; i < count; i++)
                                if (d.out[(size_t)i] != want[(size_t)i] || d.adv[(size_t)i] != adv[(size_t)i]) {
                                    printf("%s: S %d W %d T %d walk %d guard %d: draw %ld is %ld after %d, expected %ld after %ld\n", argv[f], S, W, T, walk, g, i,
                                           d.out[(size_t)i], d.adv[(size_t)i], want[(size_t)i], adv[(size_t)i]);
                                    return 1;
                                }
                            if ((long)d.consumed != consumed) {
                                printf("%s: S %d W %d T %d walk %d guard %d: consumed %ld, expected %ld\n", argv[f], S, W, T, walk, g, (long)d.consumed, consumed);
                                return 1;
                            }
                            if (walk && d.recovered) return 1;
                            recovered += d.recovered;
                            combos++;
                        }
        printf("%s %d %ld %ld %ld %ld\n", argv[f], combos, recovered, branch[0], branch[1], branch[2]);
    }
    return 0;
}
