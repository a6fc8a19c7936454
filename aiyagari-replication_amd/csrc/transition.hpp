// Launch interface of the transition-path kernels (transition_kernels.hip): the backward EGM pass
// and the forward histogram pass of a perfect-foresight (MIT shock) transition, C price paths per
// launch, one workgroup per path.  Arrays [C][...] hold path c's block at c · (the block's size).
#pragma once
#include <hip/hip_runtime.h>

#include "dist.hpp"
#include "egm.hpp"

namespace aiy {

// The backward pass: from pc_T, t = T−1 … 0, the two-rate EGM step
//   RHS(j,a) = Σ_m ((β(1+r[t+1]))·P(j,m))·u'(pc_{t+1}(m,a)),  c̃ = RHS^(−1/σ),
//   â = ((c̃ + a) − w[t]·s_j)/(1 + r[t]),  g = interp1(â_j, a, a),  g < amin → amin,
//   pk_t = g,  pc_t = ((1 + r[t])·a + w[t]·s_j) − g
// — egm_fused_kernel's operations with r split into r[t+1] (the Euler equation) and r[t].
struct EgmBackwardArgs {
    int N, Na, C, T;
    int ns;  // as EgmArgs
    double beta, sigma, amin;
    const double* r;    // device [C][T+1]; r[c][T] is the terminal rate
    const double* w;    // device [C][T]
    const double* pcT;  // device [C][N][Na], or one [N][Na] for every path (pcT_stride = 0)
    size_t pcT_stride;  // N·Na or 0
    const double* a;
    const double* s;
    const double* P;
    double* pk;   // device [C][T][N][Na]
    double* pc;   // device [C][T][N][Na] (nullable)
    int* status;  // device [C]: 0 ok, 1 = â not increasing at period fail_t (periods below it
                  // are not computed; the period's own outputs are undefined)
    int* fail_t;  // device [C]: −1, or the period that stopped the path
    // the labour pass only (launch_labor_egm_backward_batch)
    double phi, theta;
    double* pl;  // device [C][T][N][Na]
    // Paths of several economies in one launch (launch_egm_backward_batch only; all zero: one
    // economy, as above).  group > 0: path c belongs to economy e = c / group and reads
    // a + e·a_stride, s + e·s_stride, P + e·P_stride and pcT + c·pcT_stride + e·pcT_estride;
    // prm (nullable) is device [C/group][3], economy e's (β, σ, amin), which then replace beta,
    // sigma and amin, with ns = is_int_ge(σ, 1) ? (int)σ : 0 formed per economy.
    int group;
    size_t a_stride, s_stride, P_stride, pcT_estride;
    const double* prm;
};
inline bool egm_backward_fits(int64_t N, int64_t Na) { return egm_batch_fits(N, Na, false); }
int launch_egm_backward_batch(const EgmBackwardArgs& A, hipStream_t st);

// The backward pass of the endogenous-labour economy (A5): the two-rate labour step
//   RHS, c̃ as above,  ℓ̃ = labor_dev(c̃, w[t]·s_j),  â = ((c̃ + a) − (w[t]·s_j)·ℓ̃)/(1 + r[t]),
//   g = interp1(â_j, c̃_j, a),  a < amin → g = amin,  pc_t = g,  pl_t = labor_dev(g, w[t]·s_j),
//   k = ((1 + r[t])·a + (w[t]·s_j)·pl_t) − g,  pk_t = k < 0 ? 0 : k
// — egm_fused_kernel's labour operations with r split in two.  LDS as egm_solve_batch_kernel<true>:
// policy_c, â and c̃ [N][Na] each (a_grid is read from global memory).
inline bool labor_egm_backward_fits(int64_t N, int64_t Na) { return egm_batch_fits(N, Na, true); }
int launch_labor_egm_backward_batch(const EgmBackwardArgs& A, hipStream_t st);

// The forward pass: from λ₀, t = 0 … T−1: the lottery plan of pk_t, K[t] = Σ λ_t·a, one push.
struct DistForwardArgs {
    int N, Na, C, T;
    const double* pk;    // device [C][T][N][Na]
    const double* lam0;  // device [C][N][Na], or one [N][Na] for every path (lam0_stride = 0)
    size_t lam0_stride;  // N·Na or 0
    const double* a;
    const double* P;     // row-major
    double* K;           // device [C][T+1]
    double* lamT;        // device [C][N][Na] (nullable)
    int* status;         // device [C]: 0 ok, 2 = pk_t's keys not monotone at period fail_t (K up
                         // to fail_t is written, the rest NaN, lamT = λ at fail_t)
    int* fail_t;         // device [C]
    const int* skip;     // device [C] (nullable): a non-zero entry — the backward pass's status —
                         // leaves the path alone but for K, all NaN; status and fail_t not written
    // the pass with hours only (launch_labor_dist_forward_batch): H[c][t] = Σ λ_t·(s_j·pl_t),
    // t = 0 … T−1, in K[t]'s summation order; NaN where K[t] is NaN
    const double* pl;    // device [C][T][N][Na]
    const double* s;     // device [N]
    double* H;           // device [C][T]
    // Paths of several economies in one launch (all zero: one economy, as above).  group > 0:
    // path c belongs to economy e = c / group and reads a + e·a_stride, P + e·P_stride and
    // lam0 + c·lam0_stride + e·lam0_estride.  (The pass with hours reads one s for all.)
    int group;
    size_t a_stride, P_stride, lam0_estride;
};
// LDS of one workgroup: dist_solve_batch_kernel<true>'s (λ, mass, lottery weights, run offsets,
// scratch) and a_grid.  The period's keys and the partial sums of K live in the mass array, which
// is dead while the plan is built.
inline size_t dist_forward_lds_bytes(int64_t N, int64_t Na) {
    return dist_batch_lds_bytes(N, Na, true) + sizeof(double) * (size_t)Na;
}
// dist_batch_fits for the lottery case, with a_grid's Na doubles on top
inline bool dist_forward_fits(int64_t N, int64_t Na) {
    return dist_batch_fits(N, Na, true) && dist_forward_lds_bytes(N, Na) <= kDistBatchMaxLds;
}
int launch_dist_forward_batch(const DistForwardArgs& A, hipStream_t st);
// The pass with hours: the same LDS and s [16] after a_grid.  The block sums of H follow those of
// K in the mass array's spare half (2·⌈n/256⌉ <= ⌊n/2⌋ from n = 4 on); at n < 4 the one block sum
// of H sits in the scratch's unused key slot.
inline size_t labor_dist_forward_lds_bytes(int64_t N, int64_t Na) {
    return dist_forward_lds_bytes(N, Na) + sizeof(double) * 16;
}
inline bool labor_dist_forward_fits(int64_t N, int64_t Na) {
    return dist_forward_fits(N, Na) && labor_dist_forward_lds_bytes(N, Na) <= kDistBatchMaxLds;
}
int launch_labor_dist_forward_batch(const DistForwardArgs& A, hipStream_t st);

}  // namespace aiy
