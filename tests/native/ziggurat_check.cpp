// ziggurat_check.cpp -- the host-compilable core of ziggurat.hip (csrc/ziggurat_core.h) against vectors of the integer restatement
// (tests/noise_reference.py), as a stand-alone program for the sanitizers: tests/test_noise_host.py builds it with
// -fsanitize=address,undefined, writes the vectors and runs it.
//
//   ziggurat_check FILE...   a file: int64 nraw, count, consumed; uint64 raw[nraw]; double draws[count]
//
// Every file is drawn in tiles of 4, 8, ..., 2048 positions; draws (bit for bit, the tail draws too: this is the host's libm on both
// sides), the consumed count and the tail list are compared.  One line a file: its name, the tile sizes run, the slow and tail counts.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ziggurat_tables.h"
#include "ziggurat_core.h"

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
        std::vector<double> want((size_t)count);
        if (fread(raw.data(), 8, (size_t)nraw, fp) != (size_t)nraw || fread(want.data(), 8, (size_t)count, fp) != (size_t)count) return 2;
        fclose(fp);
        long slow = -1, tails = -1;
        int sizes = 0;
        for (int P = 4; P <= 2048; P *= 2, sizes++) {
            const ZigDraws d = zig_draws(raw.data(), nraw, count, P, ZIG_WI, (const uint64_t *)ZIG_KI, ZIG_FI, ZIG_GUARD);
            if (d.undecided || d.short_of_outputs) {
                printf("%s: tile %d undecided %d short %d\n", argv[f], P, (int)d.undecided, (int)d.short_of_outputs);
                return 1;
            }
            if (count && memcmp(d.out.data(), want.data(), (size_t)count * 8) != 0) {
                long i = 0;
                while (memcmp(&d.out[(size_t)i], &want[(size_t)i], 8) == 0) i++;
                printf("%s: tile %d draw %ld is %a, expected %a\n", argv[f], P, i, d.out[(size_t)i], want[(size_t)i]);
                return 1;
            }
            if ((long)d.consumed != consumed) {
                printf("%s: tile %d consumed %ld, expected %ld\n", argv[f], P, (long)d.consumed, consumed);
                return 1;
            }
            for (size_t j = 0; j < d.tail_idx.size(); j++) {  // the tail list leads back to the value
                const double xx = -ZIG_INV_R * log1p(-zig_uniform(d.tail_raw[2 * j + 1]));
                const double v = ((d.tail_raw[2 * j] >> 17) & 1) ? -(ZIG_R + xx) : ZIG_R + xx;
                if (memcmp(&v, &want[(size_t)d.tail_idx[j]], 8) != 0) {
                    printf("%s: tile %d tail entry %zu does not give draw %ld\n", argv[f], P, j, d.tail_idx[j]);
                    return 1;
                }
            }
            if (slow >= 0 && (slow != d.slow || tails != (long)d.tail_idx.size())) {
                printf("%s: tile %d counts %ld slow, %zu tails differ from the tile before\n", argv[f], P, d.slow, d.tail_idx.size());
                return 1;
            }
            slow = d.slow;
            tails = (long)d.tail_idx.size();
        }
        printf("%s %d %ld %ld\n", argv[f], sizes, slow, tails);
    }
    return 0;
}
