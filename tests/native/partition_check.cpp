// partition_check.cpp -- csrc/partition_core.h as host code against plain loops: the visiting order of coadd.py:331-341 for sparse axes whose
// cells are ragged (np.linspace(0, nside, sp_res + 1, dtype=np.uint16) truncates), with empty cells, a single cell and irrelevant cells.
// Prints one line a case: name, visits checked, mismatches.  Built with the host sanitizers by tests/test_inpool_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "partition_core.h"

using namespace imcom;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned int rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned int)(rng_state >> 33);
}

// every `keep_of`-th cell in `keep_of + 1` is relevant (0: all)
static int run(const char *name, int nside, int sp_res, int drop_one_in)
{
    std::vector<unsigned short> sp(sp_res + 1);
    for (int k = 0; k <= sp_res; k++) sp[k] = (unsigned short)((double)nside * k / sp_res);  // the truncation of the uint16 linspace
    sp[sp_res] = (unsigned short)nside;
    std::vector<unsigned char> rel((size_t)sp_res * sp_res);
    for (auto &r : rel) r = drop_one_in == 0 || rnd() % drop_one_in != 0;
    std::vector<unsigned int> start((size_t)sp_res * sp_res + 1), cell((size_t)sp_res * sp_res);
    const int ncell = partition_cells(sp.data(), rel.data(), sp_res, start.data(), cell.data());
    long p = 0, bad = 0;
    for (int j = 0; j < sp_res; j++)
        for (int i = 0; i < sp_res; i++) {
            if (!rel[(size_t)j * sp_res + i]) continue;
            for (int y = sp[j]; y < sp[j + 1]; y++)
                for (int x = sp[i]; x < sp[i + 1]; x++, p++) {
                    if (p >= (long)start[ncell]) {
                        bad++;
                        continue;
                    }
                    int gy = -1, gx = -1;
                    partition_decode(start.data(), cell.data(), ncell, sp.data(), sp_res, (unsigned int)p, &gy, &gx);
                    if (gy != y || gx != x) bad++;
                }
        }
    if (p != (long)start[ncell]) bad++;
    printf("%s %ld %ld\n", name, p, bad);
    return bad != 0;
}

int main()
{
    int fail = 0;
    fail |= run("ragged_190_8", 190, 8, 3);
    fail |= run("ragged_190_24", 190, 24, 4);
    fail |= run("all_190_8", 190, 8, 0);
    fail |= run("sca_4088_90", 4088, 90, 5);
    fail |= run("empty_cells_5_8", 5, 8, 0);
    fail |= run("single_cell", 37, 1, 0);
    fail |= run("sparse_1000_90", 1000, 90, 1);  // (drop_one_in = 1: nothing is relevant)
    return fail;
}
