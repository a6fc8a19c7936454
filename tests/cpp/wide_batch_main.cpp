// Stand-alone host program around the index arithmetic of the batched small-grid labour sweep
// (csrc/wide_batch.hpp): the slot-set rotation and the workgroup -> (candidate, tile item) map.
// Built with -fsanitize=address,undefined by tests/test_labor_batch_cpu.py and run without a GPU.
// It replays the host loop's launches over a model of the slot words and checks, for every
// sweep, that the set written is not the one read, that the set cleared is neither, that the set
// read is the one the previous sweep wrote and holds only that sweep's marks, and that the grid
// covers every (candidate, item) exactly once and nothing else.
#include <cstdio>
#include <vector>

#include "wide_batch.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using namespace aiy;

static void rotation(int C, int nslots, long long sweeps) {
    // slots[c][set][2 * nslots]: each word holds the sweep that last wrote it (0 = clear)
    std::vector<long long> slots(wide_batch_set_off(C, 0, nslots), 0);
    for (long long g = 1; g <= sweeps; ++g) {
        const int wr = wide_batch_write_set(g), rd = wide_batch_read_set(g),
                  cl = wide_batch_clear_set(g);
        CHECK(wr != rd && wr != cl && rd != cl);
        CHECK(wr >= 0 && wr < kWideBatchSets && rd >= 0 && rd < kWideBatchSets);
        CHECK(rd == wide_batch_write_set(g - 1) || g == 1);
        CHECK(cl == wide_batch_write_set(g + 1));
        for (int c = 0; c < C; ++c) {
            long long* r = slots.data() + wide_batch_set_off(c, rd, nslots);
            long long* w = slots.data() + wide_batch_set_off(c, wr, nslots);
            long long* k = slots.data() + wide_batch_set_off(c, cl, nslots);
            CHECK(wide_batch_set_off(c, kWideBatchSets - 1, nslots) + wide_batch_set_words(nslots) <=
                  slots.size());
            for (size_t q = 0; q < wide_batch_set_words(nslots); ++q) {
                CHECK(r[q] == g - 1);  // the previous sweep's marks only (sweep 1: clear)
                CHECK(w[q] == 0);      // cleared since its last use
            }
            for (size_t q = 0; q < wide_batch_set_words(nslots); ++q) w[q] = g, k[q] = 0;
        }
    }
}

static void blocks(int C, int N, int Na, int SB) {
    const int ntile = wide_batch_ntile(Na, SB), bpc = wide_batch_bpc(N, ntile);
    const int grid = wide_batch_grid(C, bpc);
    CHECK(ntile * SB >= Na && (ntile - 1) * SB < Na);
    CHECK(grid == C * bpc);
    std::vector<int> seen((size_t)C * N * ntile, 0);
    for (int b = 0; b < grid; ++b) {
        const WideBatchBlock wb = wide_batch_block(b, bpc);
        CHECK(wb.c >= 0 && wb.c < C && wb.item >= 0 && wb.item < N * ntile);
        const int i = wb.item / ntile, tile = wb.item % ntile;
        CHECK(i < N && tile * SB < Na);
        ++seen[(size_t)wb.c * N * ntile + wb.item];
    }
    for (int v : seen) CHECK(v == 1);
    // each candidate's first workgroup (it records the stop and clears the next set) is item 0
    for (int c = 0; c < C; ++c) CHECK(wide_batch_block(c * bpc, bpc).item == 0);
}

int main() {
    for (int C : {1, 2, 7, 70}) rotation(C, 64, 50);
    rotation(3, 1, 7);
    for (int C : {1, 2, 7, 70})
        for (int SB : {8, 16, 32, 64}) {
            blocks(C, 1, 2, SB);
            blocks(C, 2, 3, SB);
            blocks(C, 7, 63, SB);
            blocks(C, 7, 65, SB);
            blocks(C, 16, 128, SB);
            blocks(C, 7, 400, SB);
        }
    // a grid past 2^31 - 1 blocks is refused, the largest that fits is not
    CHECK(wide_batch_grid(1ll << 20, 7 * 512) == 0);
    CHECK(wide_batch_grid(1ll << 20, 2047) == (int)((1ll << 20) * 2047));
    CHECK(wide_batch_grid(1ll << 20, 2048) == 0);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("done\n");
    return 0;
}
