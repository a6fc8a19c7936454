// Launch interface of the sequence-space Jacobian kernels (ssj_kernels.hip): the expectation
// vectors of a constant policy (the transposed push, T − 1 dependent steps in one workgroup) and
// the fake-news contraction with its diagonal accumulation (Auclert, Bardóczy, Rognlie, Straub
// 2021).  Arrays [C][...] hold block c at c · (the block's size); n = N·Na.
#pragma once
#include <hip/hip_runtime.h>

#include "dist.hpp"

namespace aiy {

// Expectation vectors of the policy g [N][Na] and the outcome y₀ [N][Na].  The plan is
// dist_keys_kernel's: x = g clamped to [a₀, a_last], lo = its bracket, wr = (x − a[lo]) /
// (a[lo+1] − a[lo]); wl = 1 − wr is the weight on the lower node.  E₀ = y₀ and, t = 0 … T−2,
//   G_t(i, k′)   = Σ_m P(i, m)·E_t(m, k′)                         (m ascending, from +0)
//   E_{t+1}(i,k) = wl(i,k)·G_t(i, lo(i,k)) + (1 − wl(i,k))·G_t(i, lo(i,k) + 1)
// — the transpose of dist_solve_batch_kernel<true>'s push: E_t·λ₀ = y₀·λ_t.
struct DistExpectArgs {
    int N, Na, C, T;
    const double* pk;   // device [C][N][Na]
    const double* y0;   // device [C][N][Na], or one [N][Na] for every c (y0_stride = 0)
    size_t y0_stride;   // N·Na or 0
    const double* a;
    const double* P;    // row-major
    double* E;          // device [C][T][N][Na]
    // One economy per steady state (all zero: one economy, as above): c reads its policy at
    // pk + c·pk_stride (pk_stride = 0: N·Na), a + c·a_stride and P + c·P_stride.
    size_t pk_stride, a_stride, P_stride;
};
// LDS of one workgroup: E_t, G_t, wl (N·Na doubles each), lo (N·Na ints, padded to 8 bytes) and
// P [16][16].  a_grid sits in G's array while the plan is built.
inline size_t dist_expect_lds_bytes(int64_t N, int64_t Na) {
    const size_t n = (size_t)N * Na;
    return sizeof(double) * 3 * n + sizeof(int) * ((n + 1) & ~(size_t)1) + sizeof(double) * 256;
}
// N·Na = 2,800 (the scripts' grid): 80 KB
inline bool dist_expect_fits(int64_t N, int64_t Na) {
    return N >= 1 && N <= kDistPushMaxN && Na >= 2 &&
           dist_expect_lds_bytes(N, Na) <= kDistBatchMaxLds;
}
int launch_dist_expect_batch(const DistExpectArgs& A, hipStream_t st);

// The fake-news matrices and the Jacobians of n_in inputs: with D_x[s] = (Λ1[x+1][T−1−s] −
// Λ1[0][T−1−s]) / h (one subtraction, one division per element, never stored),
//   F[x][t][s] = Σ_k E[t][k]·D_x[s][k]                 (fp64 MFMA, k ascending in steps of 4)
//   J[x][t][s] = F[x][t][s] + J[x][t−1][s−1]  (t, s >= 1; = F on the first row and column)
struct SsjFakeNewsArgs {
    int T, n_in, n;
    double h;
    const double* E;     // device [T][n]
    const double* lam1;  // device [n_in + 1][T][n], block 0 the base
    double* F;           // device [n_in][T][T]
    double* J;           // device [n_in][T][T]
    // C economies in one launch (C = 0: one, as above): E [C][T][n], lam1 [C][n_in + 1][T][n],
    // F and J [C][n_in][T][T]; the launch grid's third dimension is c·n_in + x, so C·n_in <=
    // 65,535.  An entry's MFMA chain is the same whatever C.
    int C;
};
constexpr int kSsjMaxT = 32768;  // T·T entries and the launch grid stay below 2^31 / 65,536
// economies per chunk of aiy_ssj_jacobian_batch: 2 inputs each in the grid's third dimension
constexpr int64_t kSsjBatchMaxChunk = 32767;
int launch_ssj_fake_news(const SsjFakeNewsArgs& A, hipStream_t st);

// The labour economy's hours H_t = Σ λ_t·(s_j·pl_t) respond to news at date 0 already (the policy
// pl_0 itself moves), which the capital path does not.  y [N][Na] = s_j·pl(j,a) is the outcome
// whose expectation vectors E^h carry the response through the distribution;
int launch_ssj_hours_outcome(const double* s, const double* pl, int N, int Na, double* y,
                             hipStream_t st);
// with G = E^h·D_xᵀ (the fake-news contraction, unchanged) and H1 [n_in+1][T] the hours of the
// one-step pushes (block 0 the base),
//   F_H[x][0][s] = (H1[x+1][T−1−s] − H1[0][T−1−s]) / h,   F_H[x][t][s] = G[x][t−1][s]  (t >= 1),
//   J_H[x][t][s] = F_H[x][t][s] + J_H[x][t−1][s−1]   (ssj_jacobian_kernel, unchanged).
struct SsjHoursArgs {
    int T, n_in, n;
    double h;
    const double* Eh;    // device [T][n]
    const double* lam1;  // device [n_in + 1][T][n]
    const double* H1;    // device [n_in + 1][T]
    double* G;           // device [n_in][T][T] (scratch)
    double* F;           // device [n_in][T][T]
    double* J;           // device [n_in][T][T]
};
int launch_ssj_hours_jacobian(const SsjHoursArgs& A, hipStream_t st);

}  // namespace aiy
