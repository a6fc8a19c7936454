// F2 histogram — the non-stochastic simulation (Young 2010) of the Krusell-Smith capital path
// (new; the reference simulates a panel of agents, Krusell_Smith_VFI.m:206-248).
// A distribution λ_t over (employment e, node j of a histogram grid x) is pushed through one
// aggregate shock path with the period's policy k_opt(., K_t, (z_t, e)); K_t is its first
// moment.  The state is 2·nx numbers, so the whole T-period recursion of a path runs in ONE
// workgroup from LDS, and M independent paths are M workgroups of one launch.  No workgroup
// waits for another: no grid barrier, no atomics, every loop bounded by T, nx or log2 nx, and
// every segment search clamps its result, so no operand value can index out of range.
//
// Fit rule (ks_hist.hpp ks_hist_fits): nx >= 2, nk >= 2, nK >= 2 and
//   8·(8·nx + nK + 8) + 4·(5·nx + 4)  <=  160 KiB          (nx = 1,000, nK = 4: 84 KB);
// k_opt (8·4·nK·nk bytes) joins it in LDS when the sum still fits (the reference's 100 x 4 x 4:
// 97 KB), otherwise it is read through L2.
// LDS (dynamic, 16-byte aligned base): λ [2][nx], pushed mass [2][nx], lottery weights [2][nx],
// x [nx], tk_j [nx], K_grid [nK], 8 slots of wave sums, k_opt [4][nK][nk] (when staged); then the
// ints: keys [2][nx], run offsets [2][nx+1], ik_j [nx], the vote's two words.  (ik_j, tk_j) = segment and weight of
// x[j] in k_grid, computed once per call with the panel's operations.
//
// A period is five phases, one barrier after each:
//   1. moment   K_t = Σ λ[e][j]·x[j] over the flat index f = e·nx + j: thread l < 256 sums
//               f = l, l + 256, ... in order; each of the four waves folds its 64 sums pairwise
//               (h = 32 ... 1: s[l] + s[l+h]); K_t = (q0 + q2) + (q1 + q3) of the wave sums q.
//               K_t is not normalised by Σ λ.
//   2. keys     segment iK / weight tK of K_t in K_grid (clamped to [0, nK-2]: linear
//               extrapolation), then per source (e, j): kn = the panel's bilinear move at
//               (ik_j, tk_j, iK, tK, s = 2·z_t + e), clamped to [x[0], x[nx-1]]; key = its
//               segment in x (<= nx-2), w = (kn - x[key]) / (x[key+1] - x[key]).
//   3. offsets  off(e, k) = #{j : key(e, j) < k} by binary search over row e's keys, and the
//               monotonicity vote: some key(e, j-1) > key(e, j) -> the whole period (both rows)
//               takes the slow path.  The policy of a period depends on K_t, so this is decided
//               per period; slow[m] counts such periods.
//   4. gather   pushed_e[j'] = Σ λ·w over key = j'-1 plus Σ λ·(1-w) over key = j'.
//               Fast path (monotone rows): the sources are the run [off(j'-1), off(j'+1)), summed
//               in the A10 order of dist_mass<true> (dist_dev.hpp): ascending j, runs longer than
//               kDistChunk by chunk, the chunk sums added in chunk order.
//               Slow path: destination j' scans all sources j = 0 ... nx-1 of its row in
//               ascending j and adds the matching terms one after another, from 0.0.
//   5. mix      λ_{t+1}[e'][j'] = p(e'|0)·pushed_0[j'] + p(e'|1)·pushed_1[j'], accumulated from
//               0.0 in e order; p(0|e) = thr[(z_{t+1}·2 + z_t)·2 + e], p(1|e) = 1 - p(0|e) — the
//               table ks_eps_kernel draws the panel's employment chain from.
// After the loop K_ts[T-1] is the moment of λ_{T-1}, which is returned.  tests/ks_hist_ref.py
// restates every addition above in numpy.
#include "aiy_common.hpp"
#include "dist_dev.hpp"
#include "ks_hist.hpp"

#include <algorithm>

namespace aiy {

// ks_panel_step_kernel's move_agent on a k_opt base pointer (global or LDS)
__device__ __forceinline__ double hist_move(const double* ko, int nk, int nK, int iK, double tK,
                                            int s, int ik, double tk) {
    const double* f = ko + ((size_t)s * nK + iK) * nk + ik;
    const double f00 = f[0], f10 = f[1], f01 = f[nk], f11 = f[nk + 1];
    const double f0 = f00 + tk * (f10 - f00);
    const double f1 = f01 + tk * (f11 - f01);
    return f0 + tK * (f1 - f0);
}

// phase 1 up to its barrier: the wave sums of Σ λ·x into s_q[0..3]
__device__ __forceinline__ void hist_moment(const double* s_lam, const double* s_x, int nx,
                                            double* s_q) {
    const int tid = threadIdx.x;
    if (tid < kHistFold) {
        double acc = 0.0;
        int j = tid % nx;
        const int dj = kHistFold % nx;
        for (int f = tid; f < 2 * nx; f += kHistFold) {
            acc = acc + s_lam[f] * s_x[j];
            j += dj;
            j = j >= nx ? j - nx : j;
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
            const double o = __shfl_down(acc, h);
            acc = acc + o;  // lanes l < h hold s[l] + s[l+h]
        }
        if ((tid & 63) == 0) s_q[tid >> 6] = acc;
    }
}

// MULTI: path m runs its own candidate c = A.pol[m] — k_opt block c, K_grid row c and the
// employment table A.thr_g + 8·c (read from global memory in phase 5); everything else, the
// LDS map included, is the single-policy kernel's.
template <bool KLDS, bool MULTI>
__global__ __launch_bounds__(1024) void ks_hist_sim_kernel(HistArgs A) {
    extern __shared__ __align__(16) unsigned char ks_hist_lds[];
    const int m = blockIdx.x;  // (the grid is exactly M workgroups)
    const int nx = A.nx, nk = A.nk, nK = A.nK, T = A.T, n = 2 * nx, W = nx + 1;
    double* const s_lam = reinterpret_cast<double*>(ks_hist_lds);
    double* const s_push = s_lam + n;
    double* const s_w = s_push + n;
    double* const s_x = s_w + n;
    double* const s_tk = s_x + nx;
    double* const s_Kg = s_tk + nx;
    double* const s_q = s_Kg + nK;
    double* const s_ko = s_q + 8;
    int* const s_key = reinterpret_cast<int*>(s_ko + (KLDS ? 4 * nK * nk : 0));
    int* const s_off = s_key + n;
    int* const s_ik = s_off + 2 * W;
    int* const s_vote = s_ik + nx;  // [2]: period t votes in word t & 1

    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const double* __restrict__ kg = A.k_grid;
    double* __restrict__ lam_g = A.lam + (size_t)m * n;
    const int8_t* __restrict__ zi = A.zi + (size_t)m * T;
    double* __restrict__ Kts = A.K_ts + (size_t)m * T;
    const int cand = MULTI ? A.pol[m] : 0;
    const double* __restrict__ ko_g = A.k_opt + (size_t)cand * 4 * nK * nk;
    const double* __restrict__ Kg_g = A.K_grid + (size_t)cand * nK;
    const double* __restrict__ thr_c = MULTI ? A.thr_g + 8 * (size_t)cand : nullptr;

    for (int j = tid; j < nx; j += nthr) {
        const double xj = A.x[j];
        const int ik = seg_of_dev(kg, nk, xj);
        s_x[j] = xj;
        s_ik[j] = ik;
        s_tk[j] = (xj - kg[ik]) / (kg[ik + 1] - kg[ik]);
    }
    for (int q = tid; q < nK; q += nthr) s_Kg[q] = Kg_g[q];
    if (tid < 2) s_vote[tid] = 0;
    for (int f = tid; f < n; f += nthr) s_lam[f] = lam_g[f];
    if (KLDS)
        for (int q = tid; q < 4 * nK * nk; q += nthr) s_ko[q] = ko_g[q];
    const double* ko = KLDS ? s_ko : ko_g;
    __syncthreads();

    const double x0 = s_x[0], xn = s_x[nx - 1];
    // element f = e·nx + j of this thread's strided walk, without a division per element
    const int e0 = tid / nx, j0 = tid - e0 * nx;
    const int de = nthr / nx, dj = nthr - de * nx;
    long long slow = 0;
    int zt = zi[0] != 0;  // (a shock code indexes k_opt and thr: kept in {0, 1})
    int z1 = zi[1] != 0;

    for (int t = 0; t + 1 < T; ++t) {
        const int zn = z1;
        z1 = zi[t + 2 < T ? t + 2 : T - 1] != 0;  // next period's, loaded a period ahead
        hist_moment(s_lam, s_x, nx, s_q);  // phase 1
        __syncthreads();
        const double K = (s_q[0] + s_q[2]) + (s_q[1] + s_q[3]);
        if (tid == 0) Kts[t] = K;
        {  // phase 2
            const int iK = seg_of_dev(s_Kg, nK, K);
            const double tK = (K - s_Kg[iK]) / (s_Kg[iK + 1] - s_Kg[iK]);
            int e = e0, j = j0;
            for (int f = tid; f < n; f += nthr) {
                double kn = hist_move(ko, nk, nK, iK, tK, 2 * zt + e, s_ik[j], s_tk[j]);
                kn = kn < x0 ? x0 : kn;
                kn = kn > xn ? xn : kn;
                const int key = seg_of_dev(s_x, nx, kn);
                s_key[f] = key;
                s_w[f] = (kn - s_x[key]) / (s_x[key + 1] - s_x[key]);
                j += dj;
                e += de;
                if (j >= nx) {
                    j -= nx;
                    ++e;
                }
            }
        }
        __syncthreads();
        if (tid == 0) s_vote[(t + 1) & 1] = 0;  // the next period's word (last read a period ago)
        for (int q = tid; q < 2 * W; q += nthr) {  // phase 3
            const int e = q >= W ? 1 : 0, k = q - e * W;
            const int* row = s_key + e * nx;
            if (k >= 1 && k < nx && row[k - 1] > row[k]) s_vote[t & 1] = 1;  // (all write 1)
            int lo = 0, hi = nx;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (row[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            s_off[q] = lo;
        }
        __syncthreads();
        const int slow_period = s_vote[t & 1];  // workgroup-uniform
        if (!slow_period) {
            // phase 4, fast: the wave's trip count is uniform (dist_mass is wave-cooperative)
            int e = e0, k = j0;
            for (int fb = tid - lane; fb < n; fb += nthr) {
                const int f = fb + lane;
                int jb = 0, js = 0, je = 0;  // a lane past the end: an empty run
                if (f < n) {
                    const int* o = s_off + e * W;
                    const int r0 = e * nx;
                    js = o[k] + r0;
                    je = o[k + 1] + r0;
                    jb = k > 0 ? o[k - 1] + r0 : js;
                }
                const double tot = dist_mass<true>(s_lam, s_w, jb, js, je, 0);
                if (f < n) s_push[f] = tot;
                k += dj;
                e += de;
                if (k >= nx) {
                    k -= nx;
                    ++e;
                }
            }
        } else {
            ++slow;
            int e = e0, k = j0;
            for (int f = tid; f < n; f += nthr) {
                const int r0 = e * nx;
                double acc = 0.0;
                for (int j = 0; j < nx; ++j) {
                    const int key = s_key[r0 + j];
                    // dist_term: λ·w for a source j below js, λ·(1-w) otherwise
                    if (key == k - 1) acc = acc + dist_term<true>(s_lam, s_w, r0 + j, r0 + j + 1, 0);
                    else if (key == k) acc = acc + dist_term<true>(s_lam, s_w, r0 + j, r0 + j, 0);
                }
                s_push[f] = acc;
                k += dj;
                e += de;
                if (k >= nx) {
                    k -= nx;
                    ++e;
                }
            }
        }
        __syncthreads();
        {  // phase 5
            const int ti = (zn * 2 + zt) * 2;
            const double p0 = MULTI ? thr_c[ti] : A.thr[ti], p1 = MULTI ? thr_c[ti + 1] : A.thr[ti + 1];
            int e = e0, k = j0;
            for (int f = tid; f < n; f += nthr) {
                const double a0 = e == 0 ? p0 : 1 - p0, a1 = e == 0 ? p1 : 1 - p1;
                double acc = 0.0;
                acc = acc + a0 * s_push[k];
                acc = acc + a1 * s_push[nx + k];
                s_lam[f] = acc;
                k += dj;
                e += de;
                if (k >= nx) {
                    k -= nx;
                    ++e;
                }
            }
        }
        __syncthreads();
        zt = zn;
    }

    hist_moment(s_lam, s_x, nx, s_q);
    __syncthreads();
    if (tid == 0) {
        Kts[T - 1] = (s_q[0] + s_q[2]) + (s_q[1] + s_q[3]);
        if (A.slow) A.slow[m] = slow;
    }
    for (int f = tid; f < n; f += nthr) lam_g[f] = s_lam[f];
}

int launch_ks_hist(const HistArgs& A, hipStream_t st) {
    if (A.M < 1 || A.M > kHistMaxPaths || A.T < 2 || !ks_hist_fits(A.nx, A.nk, A.nK))
        return fail(AIY_BAD_SHAPE, "histogram simulation: need T >= 2, 1 <= M <= 65,535 and a "
                                   "path's state inside one CU's LDS");
    const bool klds = ks_hist_kopt_in_lds(A.nx, A.nk, A.nK);
    const size_t lds = ks_hist_lds_bytes(A.nx, A.nk, A.nK, klds);
    const int nthr = std::min(1024, std::max(kHistFold, (2 * A.nx + 63) & ~63));
    const bool multi = A.pol != nullptr;
#define AIY_HIST_LAUNCH(KLDS_, MULTI_)                                                          \
    do {                                                                                        \
        if (lds > 64 * 1024) /* dynamic LDS past 64 KiB needs the attribute */                  \
            AIY_TRY((raise_dynamic_lds<ks_hist_sim_kernel<KLDS_, MULTI_>>((int)kHistMaxLds)));  \
        ks_hist_sim_kernel<KLDS_, MULTI_><<<A.M, nthr, lds, st>>>(A);                           \
    } while (0)
    if (klds && multi) AIY_HIST_LAUNCH(true, true);
    else if (klds) AIY_HIST_LAUNCH(true, false);
    else if (multi) AIY_HIST_LAUNCH(false, true);
    else AIY_HIST_LAUNCH(false, false);
#undef AIY_HIST_LAUNCH
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
