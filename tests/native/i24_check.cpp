// i24_check.cpp -- i24_core.h as host code against plain loops over the same data (built by tests/test_i24_host.py with
// -fsanitize=address,undefined): the bit-stream index maps through the tiles' ownership of output bytes, the ranking of a tile's overflow
// hits, the chunked scan of tile sums and the dealing of a tile to its threads, the integer transforms.  Prints one row a family:
// name, checks made, failures.
#include <cstdio>
#include <random>
#include <vector>

#include "i24_core.h"

using namespace imcom;

static std::vector<long> sizes()
{
    std::vector<long> n;
    for (long k = 1; k <= 130; k++) n.push_back(k);
    for (long k : {I24_TILE - 1, I24_TILE, I24_TILE + 1, I24_TILE + 7, I24_TILE + 8, 2 * I24_TILE - 3, 2 * I24_TILE, 3 * I24_TILE + 5}) n.push_back(k);
    return n;
}

int main()
{
    std::mt19937 rng(24);
    long checks = 0, fails = 0;

    // the stream: every output byte has one owner tile; gathered through the windows a workgroup stages, it equals the plain definition
    for (long n : sizes()) {
        std::vector<int> code(n);
        for (auto &c : code) c = (int)(rng() & 0xffffff);
        std::vector<unsigned char> want(3 * n, 0), got(3 * n, 0);
        std::vector<int> owners(n, 0);
        for (int j = 0; j < 3; j++)
            for (long s = 0; s < 8 * n; s++) want[j * n + s / 8] |= (unsigned char)((((code[s % n] >> (8 * j)) >> (s / n)) & 1) << (s % 8));
        for (long tile = 0; tile < i24_tiles(n); tile++) {
            const long p0 = tile * I24_TILE, p1 = p0 + I24_TILE < n ? p0 + I24_TILE : n;
            for (int b = 0; b < 8; b++) {
                long k0, k1;
                i24_tile_bytes(n, p0, p1, b, &k0, &k1);
                checks++;
                if (k1 - k0 > I24_THREADS || k1 > n) fails++;
                for (long k = k0; k < k1; k++) {
                    owners[k]++;
                    const uint32_t planes = i24_gather_planes(k, n, [&](long p) {
                        const bool in_main = p >= p0 && p < p0 + I24_TILE + I24_HALO, in_wrap = p < I24_HALO;
                        if (!(in_main || in_wrap) || p >= n || p < 0) fails++;
                        return code.at(p);
                    });
                    for (int j = 0; j < 3; j++) got[j * n + k] = (unsigned char)(planes >> (8 * j));
                }
            }
        }
        for (long k = 0; k < n; k++) {
            checks++;
            if (owners[k] != 1) fails++;
        }
        for (long i = 0; i < 3 * n; i++) {
            checks++;
            if (got[i] != want[i]) fails++;
        }
        for (int j = 0; j < 3; j++)
            for (long p = 0; p < n; p++) {
                const unsigned byte = i24_scatter_byte(p, n, [&](long k) { return got.at(j * n + k); });
                checks++;
                if (byte != (unsigned)((code[p] >> (8 * j)) & 255)) fails++;
            }
    }
    printf("stream %ld %ld\n", checks, fails);

    // the ranking: (item, wave) slots, ballots and popcounts against a plain count in flat order
    checks = fails = 0;
    for (long n : {1L, 63L, 64L, 65L, 255L, 256L, 257L, (long)I24_TILE - 1, (long)I24_TILE})
        for (int density : {0, 1, 3, 50, 100}) {
            std::vector<char> hit(I24_TILE, 0);
            for (long p = 0; p < n; p++) hit[p] = (int)(rng() % 100) < density;
            unsigned slots[I24_SLOTS];
            std::vector<uint64_t> ballots(I24_SLOTS, 0);
            for (int i = 0; i < I24_ITEMS; i++)
                for (int t = 0; t < I24_THREADS; t++) {
                    const long p = i24_rank_pixel(0, i, t);
                    if (p < n && hit[p]) ballots[i24_rank_slot(i, t / I24_WAVE)] |= 1ull << (t % I24_WAVE);
                }
            for (int s = 0; s < I24_SLOTS; s++) slots[s] = (unsigned)__builtin_popcountll(ballots[s]);
            const unsigned total = i24_slot_offsets(slots);
            std::vector<long> where(I24_TILE, -1);
            for (int i = 0; i < I24_ITEMS; i++)
                for (int t = 0; t < I24_THREADS; t++) {
                    const int s = i24_rank_slot(i, t / I24_WAVE), lane = t % I24_WAVE;
                    if ((ballots[s] >> lane) & 1) where[slots[s] + i24_popcount_below(ballots[s], lane)] = i24_rank_pixel(0, i, t);
                }
            long r = 0;
            for (long p = 0; p < n; p++)
                if (hit[p]) {
                    checks++;
                    if (where[r++] != p) fails++;
                }
            checks++;
            if (total != (unsigned)r) fails++;
        }
    printf("rank %ld %ld\n", checks, fails);

    // the scan: thread-major items inside a tile, tile sums in chunks with a carry, wrapping at 2^32
    checks = fails = 0;
    for (long n : {1L, 7L, (long)I24_TILE - 1, (long)I24_TILE, (long)I24_TILE + 1, (long)I24_TILE * (2 * I24_SCAN_CHUNK + 1) + 5}) {
        std::vector<uint32_t> v(n);
        for (auto &x : v) x = (rng() % 4 == 0) ? 0xffffffu : (uint32_t)(rng() & 0xffffff);
        const long tiles = i24_tiles(n);
        std::vector<uint32_t> sums(tiles, 0), out(n);
        for (long tile = 0; tile < tiles; tile++)
            for (int t = 0; t < I24_THREADS; t++)
                for (int e = 0; e < I24_ITEMS; e++) {
                    const long p = i24_scan_pixel(tile * I24_TILE, t, e);
                    if (p < n) sums[tile] += v[p];
                }
        const uint32_t total = i24_scan_chunks(sums.data(), tiles, [&](uint32_t *chunk, int cnt, uint32_t carry) {
            if (cnt > I24_SCAN_CHUNK) fails++;
            for (int i = 0; i < cnt; i++) {
                const uint32_t c = chunk[i];
                chunk[i] = carry;
                carry += c;
            }
            return carry;
        });
        for (long tile = 0; tile < tiles; tile++) {
            uint32_t below = 0;  // (the threads below t, as the workgroup's exclusive scan gives it)
            for (int t = 0; t < I24_THREADS; t++) {
                uint32_t acc = sums[tile] + below;
                for (int e = 0; e < I24_ITEMS; e++) {
                    const long p = i24_scan_pixel(tile * I24_TILE, t, e);
                    if (p >= n) continue;
                    acc += v[p];
                    below += v[p];
                    out[p] = acc;
                }
            }
        }
        uint32_t run = 0;
        for (long p = 0; p < n; p++) {
            run += v[p];
            checks++;
            if (out[p] != run) fails++;
        }
        checks++;
        if (total != run) fails++;
    }
    printf("scan %ld %ld\n", checks, fails);

    // the integer transforms: each inverse undoes its forward on every code of a small BITKEEP and on random ones of the large
    checks = fails = 0;
    for (int B : {1, 7, 8, 9, 16, 17, 20, 23, 24}) {
        const int M = (int)((1u << B) - 1u);
        for (int k = 0; k < 4096; k++) {
            const int q = B <= 12 ? (k & M) : (int)(rng() & (uint32_t)M), prev = (int)(rng() & (uint32_t)M);
            for (int s : {0, 1, 64 & M, M, -1, -2}) {
                const int f = i24_softbias_fwd(q, B, s);
                checks++;
                if (f < 0 || f > M || i24_softbias_rev(f, B, s) != q) fails++;
            }
            const int d = i24_diff_fwd(q, prev, B);
            checks++;
            if (d < 0 || d > M || (int)(((uint32_t)d + (uint32_t)prev) & (uint32_t)M) != q) fails++;
        }
    }
    printf("ints %ld %ld\n", checks, fails);
    return 0;
}
