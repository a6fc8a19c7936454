// Launch interface of the Krusell-Smith histogram simulation (ks_hist_kernels.hip; F2
// histogram, the non-stochastic simulation of Young (2010) beside the agent panel).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace aiy {

constexpr int kHistFold = 256;                   // strided partial sums of K_t = Σ λ·x
constexpr int64_t kHistMaxPaths = 65535;         // one workgroup per path, one grid dimension
constexpr size_t kHistMaxLds = 160 * 1024;       // per CU on gfx950

// LDS of one workgroup (one shock path), in bytes.  Doubles: λ, pushed mass and lottery weights
// [2][nx] each, x [nx], tk_j [nx], K_grid [nK], the moment's wave sums (8 slots), then k_opt
// [4][nK][nk] when `kopt` is set; ints: keys [2][nx], run offsets [2][nx+1], ik_j [nx], the
// monotonicity vote's 2 words, padded to 8 bytes.  The kernel has no static LDS.
constexpr size_t ks_hist_lds_bytes(int64_t nx, int64_t nk, int64_t nK, bool kopt) {
    const size_t nd = 8 * (size_t)nx + (size_t)nK + 8 + (kopt ? 4 * (size_t)nK * (size_t)nk : 0);
    const size_t ni = (5 * (size_t)nx + 4 + 1) & ~(size_t)1;
    return sizeof(double) * nd + sizeof(int) * ni;
}
// Fit rule of the histogram simulation: the path's own state (everything but k_opt) fits one
// CU's LDS.  nx = 1,000, nK = 4: 84 KB (97 KB with the reference's 100 x 4 x 4 k_opt).
constexpr bool ks_hist_fits(int64_t nx, int64_t nk, int64_t nK) {
    return nx >= 2 && nx <= (1 << 20) && nk >= 2 && nk <= (1 << 24) && nK >= 2 &&
           nK <= (1 << 24) && ks_hist_lds_bytes(nx, nk, nK, false) <= kHistMaxLds;
}
// k_opt is staged in LDS when it fits beside the path's state, else read through L2
constexpr bool ks_hist_kopt_in_lds(int64_t nx, int64_t nk, int64_t nK) {
    return nk * nK <= (1 << 16) && ks_hist_lds_bytes(nx, nk, nK, true) <= kHistMaxLds;
}
static_assert(ks_hist_fits(1000, 100, 4) && ks_hist_kopt_in_lds(1000, 100, 4),
              "the reference size must run from LDS");

struct HistArgs {
    int nx, nk, nK, T, M;
    double thr[8];           // [z_{t+1}][z_t][e]: P(employed next | e), ks_panel_host.cpp's table
    const double* k_grid;
    const double* K_grid;
    const double* x;         // histogram grid [nx]
    const double* k_opt;     // k x K x S column-major: (ki, Ki, s) at (s*nK + Ki)*nk + ki
    const int8_t* zi;        // [M][T] 0 good / 1 bad
    double* lam;             // [M][2][nx] in/out
    double* K_ts;            // [M][T] out
    int64_t* slow;           // [M] periods on the ordered-scan path (nullable)
    // One policy per path (ks_simulate_hist_multi): path m runs candidate c = pol[m] — k_opt
    // block c of [C][4][nK][nk], K_grid row c of [C][nK] and thr_g + 8·c (the candidate's own
    // employment table, in global memory: the LDS map does not grow).  pol = nullptr: every path
    // runs the one k_opt / K_grid / thr above.
    const int32_t* pol;      // [M], each in [0, C)
    const double* thr_g;     // [C][8]
};
int launch_ks_hist(const HistArgs& A, hipStream_t st);

}  // namespace aiy
