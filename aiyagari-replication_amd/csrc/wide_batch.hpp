// Index arithmetic of the batched small-grid labour sweep (bellman_wide_batch_kernels.hip and its
// host loop, bell_labor_solve_batch_dev): which workgroup owns which (candidate, tile item), and
// which of a candidate's three max|Δv| slot sets a sweep writes, reads and clears.  Plain C++, no
// HIP: the kernel, the host loop and tests/cpp/wide_batch_main.cpp share these functions.
#pragma once
#include <stddef.h>

namespace aiy {

// Sweep g of a candidate writes set g mod 3, folds set (g − 1) mod 3 (final since the previous
// launch ended) for the candidate's own stop test, and its first workgroup clears set
// (g + 1) mod 3 — last written by sweep g − 2, last read by sweep g − 1, next written by sweep
// g + 1.  Two sets would not do: the workgroups of one launch fold the previous set while others
// of the same launch already write the current one, so the set to clear must be a third.
constexpr int kWideBatchSets = 3;
constexpr int wide_batch_write_set(long long g) { return (int)(g % kWideBatchSets); }
constexpr int wide_batch_read_set(long long g) { return (int)((g + 2) % kWideBatchSets); }
constexpr int wide_batch_clear_set(long long g) { return (int)((g + 1) % kWideBatchSets); }
// words of one set ({max bits, any} per slot) and the offset of (candidate c, set q) in
// slots [C][3][2·nslots]
constexpr size_t wide_batch_set_words(int nslots) { return 2 * (size_t)nslots; }
constexpr size_t wide_batch_set_off(long long c, int q, int nslots) {
    return ((size_t)c * kWideBatchSets + (size_t)q) * wide_batch_set_words(nslots);
}

// Workgroups per candidate: one per (row i, tile of SB states), row-major as the single-rate
// launch numbers its items (no split of the candidate range, so no padding to a multiple of 8).
constexpr int wide_batch_ntile(int Na, int SB) { return (Na + SB - 1) / SB; }
constexpr int wide_batch_bpc(int N, int ntile) { return N * ntile; }
struct WideBatchBlock {
    int c;     // candidate
    int item;  // i * ntile + tile within the candidate
};
constexpr WideBatchBlock wide_batch_block(int block, int bpc) {
    return WideBatchBlock{block / bpc, block % bpc};
}
// the launch's grid; 0 when C·N·ntile does not fit a 31-bit block index
constexpr int wide_batch_grid(long long C, int bpc) {
    return C * (long long)bpc > 0x7fffffffll ? 0 : (int)(C * bpc);
}

}  // namespace aiy
