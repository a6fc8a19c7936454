// Launch interface of the estimation kernels (lik_kernels.hip): the MA(∞) coefficients of the
// observables for C shock processes (one product with the general-equilibrium Jacobians, on the
// fp64 matrix cores) and, one workgroup per candidate, the autocovariances of those coefficients
// and the Gaussian log-likelihood of an observed panel (Auclert, Bardóczy, Rognlie, Straub 2021,
// §5).  Arrays [C][...] hold block c at c · (the block's size).
#pragma once
#include <hip/hip_runtime.h>

#include "dist.hpp"
#include "ssj.hpp"

namespace aiy {

// m[c][o][t] = Σ_s G[o][t][s]·dZ[c][s]: ssj_fake_news_kernel's tile scheme with the candidates in
// the place of E's rows and the n_o·T rows of G in the place of D's.  One entry is one chain of
// ⌈T/4⌉ MFMA steps over s ascending (s past T: zeros); it depends on row (o, t) of G and row c of
// dZ only — not on C, n_o, the tile or the run.
struct SsjMaArgs {
    int n_o, T, C;
    const double* G;   // device [n_o][T][T]
    const double* dZ;  // device [C][T]
    double* m;         // device [C][n_o][T]
};
constexpr int kLikMaxNo = 64;  // observables per call
int launch_ssj_ma_batch(const SsjMaArgs& A, hipStream_t st);

// Autocovariances and log-likelihood of candidate c, n = L·n_o, row i = t·n_o + o.  Every
// operation is rounded as written (no fused multiply-add); the operations on one element and
// their order depend on (n_o, L, T) alone — not on C, the block size or the thread that does them.
//
//  1. Γ[l][o][p] = Σ_{u=0}^{T−1−l} m[o][u+l]·m[p][u]: acc = +0; u ascending, acc = acc +
//     (m[o][u+l]·m[p][u]).  l >= T: +0.  Written to Gamma as it stands (no measurement error).
//  2. V[i][k], k <= i (packed rows, i(i+1)/2 + k): Γ[t−t′][o][p] for i = (t, o), k = (t′, p); the
//     diagonal is Γ[0][o][o] + me_var[o].  z = y (row n of the same elimination).
//  3. j = 0 … n−1: d_j = V[j][j].  !(d_j > 0): status 1, fail j, loglik NaN, d[j] = d_j and
//     d[j+1 …] NaN, stop.  Else, i = j+1 … n: w_i = V[i][j] (i = n: z_j), l_i = w_i/d_j; then
//     V[i][k] = V[i][k] − (l_i·w_k) for j < k <= i < n and z_k = z_k − (l_n·w_k) for j < k < n.
//     (z_j is final when column j starts: z = L⁻¹y.)
//  4. logdet = Σ_j aiy_log(d_j), quad = Σ_j (z_j·z_j)/d_j, each from +0 with j ascending;
//     loglik = −0.5·((n·1.8378770664093453 + logdet) + quad); status 0, fail −1.
// y == nullptr: step 1 only.
struct SsjLikArgs {
    int C, n_o, T, L;
    const double* m;       // device [C][n_o][T]
    const double* y;       // device [L][n_o], or nullptr
    const double* me_var;  // device [n_o] (me_stride 0) or [C][n_o] (me_stride n_o)
    size_t me_stride;
    double* loglik;        // device [C]
    int* status;           // device [C]
    int* fail;             // device [C]
    double* Gamma;         // device [C][L][n_o][n_o], or nullptr
    double* d;             // device [C][n], or nullptr
};
constexpr double kLog2Pi = 1.8378770664093453;
// LDS of one workgroup (doubles): the packed triangle of V — m's n_o·T values sit there while Γ is
// formed — then Γ (L·n_o²), w and l (n + 1 each) and z (n).
inline size_t lik_lds_bytes(int64_t n_o, int64_t L, int64_t T, bool factor) {
    const size_t n = (size_t)n_o * L, tri = factor ? n * (n + 1) / 2 : 0, mt = (size_t)n_o * T;
    return sizeof(double) * ((tri > mt ? tri : mt) + n * (size_t)n_o + (factor ? 3 * n + 2 : 0));
}
// n_o = 1: L <= 197; n_o = 3: L <= 65 (n = 195) while T <= n(n+1)/(2·n_o)
inline bool lik_fits(int64_t n_o, int64_t L, int64_t T) {
    return n_o >= 1 && n_o <= kLikMaxNo && L >= 1 && L <= 4096 && T >= 1 && T <= kSsjMaxT &&
           lik_lds_bytes(n_o, L, T, true) <= kDistBatchMaxLds;
}
int launch_ssj_loglik_batch(const SsjLikArgs& A, hipStream_t st);

}  // namespace aiy
