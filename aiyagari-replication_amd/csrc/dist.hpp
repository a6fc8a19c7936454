// Launch interface of the histogram kernels (dist_kernels.hip, A10).
#pragma once
#include <hip/hip_runtime.h>

namespace aiy {
// Summation order of a destination's mass (the A10 definition, restated by the C oracle
// orc_dist_*): the terms landing in (i, k), in ascending source j, are summed sequentially in
// chunks of kDistChunk consecutive terms and the chunk sums are summed sequentially.  A run of
// at most kDistChunk terms is the plain sequential sum; a long run (the borrowing constraint,
// the top of the grid) has a dependent chain of ≈ L/G + G additions instead of L.
constexpr int kDistChunk = 32;
// a push wave stages its source range in LDS when it holds at most this many sources
// (8 KB per wave on the on-grid path, 16 KB with lottery weights)
constexpr int kDistStage = 1024;
// the one-launch push (a wave per productivity state) takes N <= kDistPushMaxN; larger N run
// the per-destination run gather + projection (two launches, any N)
constexpr int kDistPushMaxN = 16;

struct DistArgs {
    int N, Na;
    bool lottery;        // off-grid policy (kp) split between bracketing nodes
    const int* idx;      // on-grid policy [N][Na], 0-based
    const double* kp;    // off-grid policy [N][Na]
    const double* a;
    const double* P;     // row-major
    const double* lam;   // [N][Na]
    double* out;         // λ' [N][Na]
    int* key;            // plan [N][Na]: destination key of source j
    int* off;            // plan [N][Na+1]: off(i,k) = #{j : key(i,j) < k} (monotone keys)
    double* wr;          // plan [N][Na]: lottery weight of the upper node
    double* mass;        // scratch [N][Na] (non-monotone fallback only)
    unsigned long long* diff;  // [2*kDiffSlots]
    unsigned* flags;     // bit 0 non-monotone policy, bit 1 index out of range
    int stage;           // push: sources a wave stages in LDS (set by launch_dist_push)
    unsigned long long* diff_clear;  // push (monotone plan): the next push's slot set, zeroed
                                     // by the first workgroup (nullable)
    long long* trace;    // (instrumentation, aiy_ws_set_timing bit 2) per-wave phase records
};
// the policy's plan (keys, lottery weights, run offsets, flags) — once per policy
int launch_dist_prepare(const DistArgs& A, hipStream_t st);
// one push λ → λ' with max|λ'−λ| into A.diff (which the caller has cleared): one fused launch
// on a monotone plan with N <= kDistPushMaxN (which also zeroes A.diff_clear), the run gather +
// projection for larger N, the ordered-scan gather + projection on a non-monotone plan
int launch_dist_push(const DistArgs& A, bool fallback, hipStream_t st);
int launch_dist_capital(const double* lam, const double* a, int N, int Na, double* part,
                        double* out, hipStream_t st);

// The batched fixed point (dist_batch_kernels.hip): candidate c's whole iteration in ONE
// workgroup, its λ, masses and plan in LDS.  Arrays [C][...] hold candidate c's block at
// c · (the block's size).
struct DistBatchArgs {
    int N, Na, C;
    bool lottery;
    double tol;
    long long max_iter;  // >= 1
    const int* idx;      // on-grid policies [C][N][Na], 0-based
    const double* kp;    // off-grid policies [C][N][Na]
    const double* a;
    const double* P;     // row-major
    const double* lam;   // [C][N][Na] the starting λ (not modified)
    double* out;         // [C][N][Na] the last push
    int* key;            // plan [C][N][Na]
    int* off;            // plan [C][N][Na+1]
    double* wr;          // plan [C][N][Na] (lottery)
    unsigned* flags;     // [C] bit 0 non-monotone policy, bit 1 index out of range (zeroed by
                         // the caller before the prepare launch); the solve, capital and fold
                         // launches leave a flagged candidate's outputs alone
    long long* iters;    // device [C]
    double* dist;        // device [C]
    double* part;        // [C][kDistCapitalBlocks] partial sums of K
    double* k;           // [C] K = Σ λ·a (nullable)
};
constexpr int kDistCapitalBlocks = 256;  // launch_dist_capital's partial sums
// LDS of one workgroup: λ and the masses (N·Na doubles each), the lottery weights (N·Na, off-grid
// policies only), the run offsets (N·(Na+1) ints, padded to 8 bytes) and the scratch (P [16][16],
// the reduction's 16 keys and flags)
constexpr size_t kDistBatchScratch = (256 + 16) * sizeof(double) + 16 * sizeof(int);
constexpr size_t kDistBatchMaxLds = 160 * 1024;  // per CU on gfx950
inline size_t dist_batch_lds_bytes(int64_t N, int64_t Na, bool lottery) {
    const size_t n = (size_t)N * Na, nw = ((size_t)N * (Na + 1) + 1) & ~(size_t)1;
    return sizeof(double) * n * (lottery ? 3 : 2) + sizeof(int) * nw + kDistBatchScratch;
}
// Fit rule of the one-launch path: the shapes of the one-launch push (N <= kDistPushMaxN: P
// and the reduction fit their fixed scratch) whose arrays fit one CU's LDS.  N = 7, Na = 400:
// 57 KB on-grid, 79 KB with lottery weights.
inline bool dist_batch_fits(int64_t N, int64_t Na, bool lottery) {
    return N >= 1 && N <= kDistPushMaxN && Na >= 2 &&
           dist_batch_lds_bytes(N, Na, lottery) <= kDistBatchMaxLds;
}
// Smallest C at which the one-launch path is the default (measured: DESIGN.md §5,
// profiles/r12_dist_batch_ab.txt); 0 = never
constexpr int64_t kDistBatchMinC = 2;
// the plans of all C candidates (keys, lottery weights, run offsets, per-candidate flags)
int launch_dist_batch_prepare(const DistBatchArgs& A, hipStream_t st);
// the solve of every unflagged candidate, then its K (A.k non-null)
int launch_dist_solve_batch(const DistBatchArgs& A, hipStream_t st);
}  // namespace aiy
