// Sequence-space Jacobian of the transition passes by the fake-news algorithm (new; the reference
// solves stationary problems only).  The backward pass gives the policies of an agent who learns
// of a price change s periods ahead and one forward push gives the distributions Λ1 they lead to
// (transition_kernels.hip); the two kernels here supply the other half.
//
// dist_expect_batch_kernel — one workgroup per steady state c, E_t, G_t, wl [N][Na] (doubles), lo
// [N][Na] (ints) and P in LDS.  The plan (dist_keys_kernel's clamp, bracket and weight) is built
// once: it is only a gather, so it needs no run offsets and no monotonicity check.  Period
// t = 0 … T−2:
//   G.  per (i, k′): G(i, k′) = Σ_m P(i, m)·E_t(m, k′), m ascending; barrier;
//   E′. per (i, k): E_{t+1}(i, k) = wl·G(i, lo) + (1 − wl)·G(i, lo + 1), to LDS (the thread's own
//       element) and to global memory; barrier.
// Exactly T − 1 steps; no convergence test, no atomics, no workgroup waits on another.
//
// ssj_fake_news_kernel — F[x] = E·D_xᵀ on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  A
// workgroup of four waves owns a 32 (t) x 32 (s) tile of one input x and walks k in chunks of 32
// staged in LDS: the E rows as they are, the D rows formed from Λ1 while the tile is loaded
// (period T−1−s, the base subtracted, divided by h).  A wave owns a 16 x 16 quarter: A = E[t][k]
// (lane l: row l & 15, k = l >> 4), B = D[s][k] (lane l: k = l >> 4, column l & 15), C/D in the
// f64 layout (column l & 15, row (l >> 4) + 4·reg).  Rows past T and k past n are zeros in LDS.
// Entry (t, s) is the chain of ⌈n/4⌉ MFMA steps over k ascending, whatever the tile it falls in,
// the other inputs or the launch: no atomics, no split of k across workgroups.
//
// ssj_jacobian_kernel — one thread per diagonal of one input: J = F + J(t−1, s−1), t ascending.
//
// Several economies in one launch (aiy_ssj_jacobian_batch): the expectation pass reads economy
// c's policy, grid and P through strides; the contraction and the diagonals take the economy in
// the grid, z = c·n_in + x, with E, Λ1, F and J blocks at c · (the block's size).  Nothing an
// entry is computed from depends on C.
#include "aiy_common.hpp"
#include "ssj.hpp"

#include <algorithm>

namespace aiy {

__global__ __launch_bounds__(1024) void dist_expect_batch_kernel(DistExpectArgs A) {
    extern __shared__ __align__(16) unsigned char dist_exp_lds[];
    const int N = A.N, Na = A.Na, n = N * Na, T = A.T;
    const int c = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, nthr = blockDim.x;
    double* const s_E = reinterpret_cast<double*>(dist_exp_lds);
    double* const s_G = s_E + n;
    double* const s_wl = s_G + n;
    double* const s_P = s_wl + n;
    int* const s_lo = reinterpret_cast<int*>(s_P + 256);

    const double* __restrict__ g = A.pk + (size_t)c * (A.pk_stride ? A.pk_stride : (size_t)n);
    const double* __restrict__ y = A.y0 + (size_t)c * A.y0_stride;
    double* __restrict__ Ec = A.E + (size_t)c * T * n;
    const double* __restrict__ P_e = A.P + (size_t)c * A.P_stride;
    const double* __restrict__ a_e = A.a + (size_t)c * A.a_stride;
    for (int q = tid; q < N * N; q += nthr) s_P[q] = P_e[q];
    for (int k = tid; k < Na; k += nthr) s_G[k] = a_e[k];  // (Na <= n: a_grid in G's array)
    for (int e = tid; e < n; e += nthr) {
        const double v = y[e];
        s_E[e] = v;
        Ec[e] = v;
    }
    __syncthreads();
    {  // the plan: dist_keys_kernel's operations, then the lower node's weight
        const double a_lo = s_G[0], a_hi = s_G[Na - 1];
        for (int e = tid; e < n; e += nthr) {
            double x = g[e];
            x = x < a_lo ? a_lo : x;
            x = x > a_hi ? a_hi : x;
            const int key = seg_of_dev(s_G, Na, x);
            const double wr = (x - s_G[key]) / (s_G[key + 1] - s_G[key]);
            s_wl[e] = 1 - wr;
            s_lo[e] = key;
        }
    }
    __syncthreads();

    // element e = i·Na + k of this thread's strided walk, without a division per element
    const int i0 = tid / Na, k0 = tid - i0 * Na;
    const int di = nthr / Na, dk = nthr - di * Na;

    for (int t = 0; t + 1 < T; ++t) {
        {  // G
            int i = i0, k = k0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int m = 0; m < N; ++m) acc = acc + s_P[i * N + m] * s_E[m * Na + k];
                s_G[e] = acc;
                k += dk;
                i += di;
                if (k >= Na) {
                    k -= Na;
                    ++i;
                }
            }
        }
        __syncthreads();
        {  // E′
            double* __restrict__ out = Ec + (size_t)(t + 1) * n;
            int i = i0, k = k0;
            for (int e = tid; e < n; e += nthr) {
                const double* __restrict__ row = s_G + i * Na;
                const int lo = s_lo[e];
                const double wl = s_wl[e];
                const double v = wl * row[lo] + (1 - wl) * row[lo + 1];
                s_E[e] = v;
                out[e] = v;
                k += dk;
                i += di;
                if (k >= Na) {
                    k -= Na;
                    ++i;
                }
            }
        }
        __syncthreads();
    }
}

typedef double ssj_v4d __attribute__((ext_vector_type(4)));
constexpr int kFnTile = 32;             // rows of E and of D per workgroup
constexpr int kFnChunk = 32;            // k per LDS stage
constexpr int kFnPitch = kFnChunk + 2;  // LDS row pitch (doubles): 34·r + q is distinct mod 32 for
                                        // the 16 rows x 2 k a ds_read_b64 lane group reads

__global__ __launch_bounds__(256) void ssj_fake_news_kernel(SsjFakeNewsArgs A) {
    __shared__ double s_e[kFnTile * kFnPitch];
    __shared__ double s_d[kFnTile * kFnPitch];
    const int T = A.T, n = A.n;
    const int c = blockIdx.z / A.n_in, x = blockIdx.z - c * A.n_in;  // (C = 0 or 1: c = 0)
    const int t0 = blockIdx.y * kFnTile, s0 = blockIdx.x * kFnTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int wt = (wave >> 1) * 16, wsd = (wave & 1) * 16;
    const double* __restrict__ Ecn = A.E + (size_t)c * T * n;
    const double* __restrict__ base = A.lam1 + (size_t)c * (A.n_in + 1) * T * n;
    const double* __restrict__ pert = base + (size_t)(x + 1) * T * n;
    // this thread's four (row, k) places of a stage: k = tid & 31, rows tid >> 5 + 8·u
    const int lk = tid & (kFnChunk - 1), lrow = tid >> 5;
    ssj_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < n; kb += kFnChunk) {
        const int k = kb + lk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = lrow + 8 * u;
            const int t = t0 + row, s = s0 + row;
            double ev = 0.0, dv = 0.0;
            if (k < n) {
                if (t < T) ev = Ecn[(size_t)t * n + k];
                if (s < T) {
                    const size_t o = (size_t)(T - 1 - s) * n + k;
                    dv = (pert[o] - base[o]) / A.h;
                }
            }
            s_e[row * kFnPitch + lk] = ev;
            s_d[row * kFnPitch + lk] = dv;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kFnChunk; kk += 4) {
            const double av = s_e[(wt + lr) * kFnPitch + kk + lq];
            const double bv = s_d[(wsd + lr) * kFnPitch + kk + lq];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int s = s0 + wsd + lr;
    double* __restrict__ Fx = A.F + (size_t)blockIdx.z * T * T;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int t = t0 + wt + lq + 4 * g;
        if (t < T && s < T) Fx[(size_t)t * T + s] = acc[g];
    }
}

// thread q of input x (of economy c: blockIdx.y = c·n_in + x): the diagonal through (max(q − (T−1), 0), max((T−1) − q, 0))
__global__ void ssj_jacobian_kernel(SsjFakeNewsArgs A) {
    const int T = A.T;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 2 * T - 1) return;
    const size_t o = (size_t)blockIdx.y * T * T;
    const double* __restrict__ F = A.F + o;
    double* __restrict__ J = A.J + o;
    int t = q > T - 1 ? q - (T - 1) : 0, s = q < T - 1 ? (T - 1) - q : 0;
    double acc = F[(size_t)t * T + s];
    J[(size_t)t * T + s] = acc;
    for (++t, ++s; t < T && s < T; ++t, ++s) {
        acc = F[(size_t)t * T + s] + acc;
        J[(size_t)t * T + s] = acc;
    }
}

// y(j, a) = s_j·pl(j, a): the hours outcome of a labour policy
__global__ void ssj_hours_outcome_kernel(const double* __restrict__ s,
                                         const double* __restrict__ pl, int n, int Na,
                                         double* __restrict__ y) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) y[e] = s[e / Na] * pl[e];
}

// F_H of input x = blockIdx.y: row 0 from the one-step hours, row t >= 1 = row t − 1 of G
__global__ void ssj_hours_rows_kernel(SsjHoursArgs A) {
    const int T = A.T;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)T * T) return;
    const int t = (int)(q / T), s = (int)(q - (size_t)t * T);
    const int x = blockIdx.y;
    const size_t o = (size_t)x * T * T;
    A.F[o + q] = t == 0 ? (A.H1[(size_t)(x + 1) * T + (T - 1 - s)] - A.H1[T - 1 - s]) / A.h
                        : A.G[o + q - T];
}

int launch_dist_expect_batch(const DistExpectArgs& A, hipStream_t st) {
    if (A.C < 1 || A.T < 1) return fail(AIY_BAD_SHAPE, "expectation pass needs C >= 1 and T >= 1");
    if (!dist_expect_fits(A.N, A.Na))
        return fail(AIY_BAD_ARG, "expectation pass: a steady state's arrays exceed one CU's LDS "
                                 "(N <= 16, 28·N·Na + 2 KB within 160 KiB)");
    const int n = A.N * A.Na;
    const int nthr = std::min(1024, std::max(64, (n + 63) & ~63));
    const size_t lds = dist_expect_lds_bytes(A.N, A.Na);
    if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
        AIY_TRY((raise_dynamic_lds<dist_expect_batch_kernel>((int)kDistBatchMaxLds)));
    dist_expect_batch_kernel<<<A.C, nthr, lds, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_ssj_fake_news(const SsjFakeNewsArgs& A, hipStream_t st) {
    if (A.T < 1 || A.T > kSsjMaxT || A.n_in < 1 || A.n_in > 65535 || A.n < 1)
        return fail(AIY_BAD_SHAPE, "fake-news contraction needs 1 <= T <= 32768, "
                                   "1 <= n_in <= 65535 and n >= 1");
    const int64_t nz = (int64_t)(A.C > 0 ? A.C : 1) * A.n_in;
    if (A.C < 0 || nz > 65535)
        return fail(AIY_BAD_SHAPE, "fake-news contraction needs C·n_in <= 65535");
    const int nt = (A.T + kFnTile - 1) / kFnTile;
    ssj_fake_news_kernel<<<dim3(nt, nt, (unsigned)nz), 256, 0, st>>>(A);
    AIY_HIP(hipGetLastError());
    ssj_jacobian_kernel<<<dim3((2 * A.T - 1 + 255) / 256, (unsigned)nz), 256, 0, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_ssj_hours_outcome(const double* s, const double* pl, int N, int Na, double* y,
                             hipStream_t st) {
    const int n = N * Na;
    if (N < 1 || Na < 1) return fail(AIY_BAD_SHAPE, "hours outcome needs N >= 1 and Na >= 1");
    ssj_hours_outcome_kernel<<<(n + 255) / 256, 256, 0, st>>>(s, pl, n, Na, y);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_ssj_hours_jacobian(const SsjHoursArgs& A, hipStream_t st) {
    if (A.T < 1 || A.T > kSsjMaxT || A.n_in < 1 || A.n_in > 65535 || A.n < 1)
        return fail(AIY_BAD_SHAPE, "hours Jacobian needs 1 <= T <= 32768, 1 <= n_in <= 65535 "
                                   "and n >= 1");
    SsjFakeNewsArgs B{};
    B.T = A.T; B.n_in = A.n_in; B.n = A.n; B.h = A.h;
    B.E = A.Eh; B.lam1 = A.lam1; B.F = A.G; B.J = A.J;
    const int nt = (A.T + kFnTile - 1) / kFnTile;
    ssj_fake_news_kernel<<<dim3(nt, nt, A.n_in), 256, 0, st>>>(B);
    AIY_HIP(hipGetLastError());
    const size_t tt = (size_t)A.T * A.T;
    ssj_hours_rows_kernel<<<dim3((unsigned)((tt + 255) / 256), A.n_in), 256, 0, st>>>(A);
    AIY_HIP(hipGetLastError());
    B.F = A.F;
    ssj_jacobian_kernel<<<dim3((2 * A.T - 1 + 255) / 256, A.n_in), 256, 0, st>>>(B);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
