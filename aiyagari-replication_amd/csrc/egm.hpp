// Launch interface of the EGM kernels (egm_kernels.hip): A4 and A5 (labor = true).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aiy_common.hpp"

namespace aiy {
struct EgmArgs {
    int N, Na;
    bool labor;
    int ns;  // sigma when sigma is an integer in [1, 63] (c^-sigma = 1/c^sigma), else 0
    double r, w, beta, sigma, amin, phi, theta;
    const double* c;  // policy_c [N][Na]
    const double* a;
    const double* s;
    const double* P;  // row-major N x N
    double* ahat;     // scratch [N][Na]
    double* cnext;    // scratch [N][Na]
    double* cout;     // policy_c_next
    double* pk;
    double* pl;       // A5 (nullable)
    unsigned long long* diff;  // [2]
    unsigned* flags;           // bit 0: a_hat not increasing (small-grid fused step: bit 1 of
                               // the diff slots' second word instead, see egm_fused_kernel)
    bool fused;                // Na <= 1024: one launch per step (egm_fused_kernel)
    unsigned long long* diff_clear;  // chain: the next step's slot set (kEgmSlotWords
                                     // words), zeroed by this launch's first workgroup (nullable)
    double* ahat_next;               // chain: step t+1's â and c̃ (the other scratch pair)
    double* cnext_next;
    int* seg;                        // [N][Na] interp1 segment of each query at the last step
                                     // (a verified hint for the next; -1 = none)
    long long* trace;                // (instrumentation, aiy_ws_set_timing bit 2) per-wave
                                     // phase records of the interp / chain kernels
};
constexpr int kEgmSlotWords = 2 * kDiffSlots + 2;  // {max bits, any} x kDiffSlots + flag word
constexpr int kEgmFusedMaxNa = 1024;  // egm_fused_kernel: one state per thread
int launch_egm_step(const EgmArgs& A, hipStream_t st);
// the chained solve (Na > 1,024): the Euler RHS of the first step, then one launch per step
// (interp1 of step t + the RHS of step t+1 on the same tiles)
int launch_egm_rhs(const EgmArgs& A, hipStream_t st);
int launch_egm_chain(const EgmArgs& A, hipStream_t st);

// The batched multi-rate solve (egm_batch_kernels.hip): candidate c's whole loop
// (Aiyagari_EGM.m:71-110, labour :64-107) in ONE workgroup, its policy_c, â and y in LDS.
struct EgmBatchArgs {
    int N, Na, C;
    bool labor;
    int ns;  // as EgmArgs
    double beta, sigma, amin, phi, theta, tol;
    long long max_iter;  // >= 1 (the host answers max_iter = 0 and tol >= 1 without a launch)
    const double* r;     // device [C]
    const double* w;     // device [C]
    const double* a;
    const double* s;
    const double* P;
    double* c;   // [C][N][Na] in: the starting policy_c, out: the last policy_c_next
    double* pk;  // [C][N][Na]
    double* pl;  // [C][N][Na] (A5, nullable)
    long long* iters;  // device [C]
    double* dist;      // device [C]
    int* status;       // device [C]: 0 ok, 1 = a non-increasing â ended the candidate's loop
};
// LDS of one workgroup: policy_c and â (N·Na each), y (a_grid: Na in A4; c̃: N·Na in A5) and the
// scratch (β(1+r)·P, w·s, the reduction's 16 keys and flags)
constexpr size_t kEgmBatchScratch = (256 + 16 + 16) * sizeof(double) + 16 * sizeof(int);
constexpr size_t kEgmBatchMaxLds = 160 * 1024;  // per CU on gfx950
inline size_t egm_batch_lds_bytes(int64_t N, int64_t Na, bool labor) {
    return sizeof(double) * (size_t)((labor ? 3 * N : 2 * N) * Na + (labor ? 0 : Na)) +
           kEgmBatchScratch;
}
// the one-launch path takes the shapes of egm_fused_kernel (one interp1 row of at most 1,024
// nodes) whose arrays fit a CU's LDS; the others run candidate after candidate
inline bool egm_batch_fits(int64_t N, int64_t Na, bool labor) {
    return N >= 1 && N <= 16 && Na >= 2 && Na <= kEgmFusedMaxNa &&
           egm_batch_lds_bytes(N, Na, labor) <= kEgmBatchMaxLds;
}
// Smallest C at which the one-launch path is the default.  Measured (profiles/
// r07_egm_batch_ab.txt): a step of the one-workgroup loop costs ~4.7 us per pass of its 1,024
// threads over the N·Na states (12.8 us at 2,800 states, 32.6 at 7,000) whatever C, a step of
// one solve after another ~10 us per candidate (the launch floor) — so C candidates win from
// C·10 >= 4.7·passes on: 2 at the scripts' grid, 4 at Na = 1,000; a single solve never does.
inline int64_t egm_batch_min_c(int64_t N, int64_t Na) {
    const int64_t passes = (N * Na + 1023) / 1024;
    return std::max<int64_t>(2, (47 * passes + 99) / 100);
}
int launch_egm_solve_batch(const EgmBatchArgs& A, hipStream_t st);
}  // namespace aiy
