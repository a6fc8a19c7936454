// A10 at many candidate policies — the whole histogram fixed point of one candidate in one
// workgroup (new; the reference has no histogram — SURVEY §8(a) A10).
// At the scripts' grid (Na = 400, N = 7) one push is a launch's fixed cost, not work, and a
// stationary distribution is a chain of ~200-1,200 pushes.  A candidate's chain fits one CU's
// LDS and the candidates of a GE round are independent, so workgroup c (up to 1,024 threads)
// runs candidate c's loop from its own λ₀ and plan with no launch, no host read and no
// speculation between pushes; a round of the bisection tree costs about its longest member.
// No workgroup waits for another: no grid barrier, no atomics, every loop bounded by max_iter.
//
// The plans of all candidates (keys, lottery weights, run offsets, flags) are built by one
// batched prepare launch pair — dist_keys_kernel and dist_offsets_kernel with a candidate
// dimension — and the host reads the C flag words once; a flagged candidate (non-monotone
// policy) is skipped by every launch here and solved by the per-candidate path.
//
// Fit rule (dist.hpp dist_batch_fits): N <= 16 and
//   8·N·Na·(2 + lottery) + 4·N·(Na+1) + 2.2 KB  <=  160 KiB.
// LDS (dynamic, 16-byte aligned base): λ [N][Na], mass [N][Na], lottery weights [N][Na]
// (off-grid policies), P [N][N] in 256 doubles, the reduction's 16 keys and 16 flags, then the
// run offsets [N][Na+1].  N = 7, Na = 400: 57 KB on-grid, 79 KB lottery.
// A push is two phases with one barrier after each:
//   1. per destination (i,k): mass(i,k) from its run(s) of λ_i in the A10 order of dist.hpp —
//      dist_mass of dist_push_kernel on the LDS rows (runs of <= 32 terms by their own lane,
//      longer runs split by chunk over the wave's lanes and folded in chunk order);
//   2. per (m,k): λ'(m,k) = Σ_i P(i,m)·mass(i,k) in i order over the thread's own λ element
//      (read first for |Δλ|), and the workgroup-wide max of |Δλ| over finite entries + the
//      "some finite" bit, as fold_slots_host reads dist_push_kernel's slots.
// The additions on every value are dist_push_kernel's, so λ, the iteration count and dist equal
// aiy_dist_stationary_dev's bit for bit; K = Σ λ·a is launch_dist_capital's sum with a
// candidate dimension (256 strided partial sums of 256 threads, pairwise block fold,
// sequential fold of the parts).
#include "aiy_common.hpp"
#include "dist.hpp"
#include "dist_dev.hpp"

#include <algorithm>

namespace aiy {

// grid (⌈N·Na / 256⌉, C): dist_keys_kernel on candidate blockIdx.y
__global__ void dist_batch_keys_kernel(DistBatchArgs A) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int Na = A.Na, n = A.N * Na;
    if (t >= n) return;
    const int c = blockIdx.y;
    const size_t g = (size_t)c * n + t;
    int key;
    if (A.lottery) {
        double x = A.kp[g];
        const double a0 = A.a[0], an = A.a[Na - 1];
        x = x < a0 ? a0 : x;
        x = x > an ? an : x;
        key = seg_of_dev(A.a, Na, x);
        A.wr[g] = (x - A.a[key]) / (A.a[key + 1] - A.a[key]);
    } else {
        key = A.idx[g];
        if (key < 0 || key >= Na) {
            atomicOr(A.flags + c, 2u);  // invalid index
            key = key < 0 ? 0 : Na - 1;
        }
    }
    A.key[g] = key;
}

// grid (⌈N·(Na+1) / 256⌉, C): dist_offsets_kernel on candidate blockIdx.y
__global__ void dist_batch_offsets_kernel(DistBatchArgs A) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int Na = A.Na, W = Na + 1;
    if (t >= A.N * W) return;
    const int c = blockIdx.y;
    const int i = t / W, k = t - i * W;
    const int* __restrict__ row = A.key + ((size_t)c * A.N + i) * Na;
    if (k >= 1 && k < Na && row[k - 1] > row[k]) atomicOr(A.flags + c, 1u);
    int lo = 0, hi = Na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    A.off[(size_t)c * A.N * W + t] = lo;
}

template <bool LOT>
__global__ __launch_bounds__(1024) void dist_solve_batch_kernel(DistBatchArgs A) {
    extern __shared__ __align__(16) unsigned char dist_batch_lds[];
    const int cand = blockIdx.x;  // (the grid is exactly C workgroups)
    if (A.flags[cand] != 0u) return;  // workgroup-uniform: the per-candidate path solves it
    const int N = A.N, Na = A.Na, n = N * Na, W = Na + 1;
    double* const s_lam = reinterpret_cast<double*>(dist_batch_lds);
    double* const s_mass = s_lam + n;
    double* const s_wr = s_mass + n;
    double* const s_P = s_wr + (LOT ? n : 0);
    unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(s_P + 256);
    int* const s_fl = reinterpret_cast<int*>(s_key + 16);
    int* const s_off = s_fl + 16;

    const size_t base = (size_t)cand * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x;
    for (int q = tid; q < N * N; q += nthr) s_P[q] = A.P[q];
    for (int e = tid; e < n; e += nthr) {
        s_lam[e] = A.lam[base + e];
        if (LOT) s_wr[e] = A.wr[base + e];
    }
    for (int q = tid; q < N * W; q += nthr) s_off[q] = A.off[(size_t)cand * N * W + q];
    __syncthreads();

    // element e = i·Na + k of this thread's strided walk, without a division per element
    const int i0 = tid / Na, k0 = tid - i0 * Na;
    const int di = nthr / Na, dk = nthr - di * Na;

    long long it = 0;
    double dist = __builtin_nan("");
    while (it < A.max_iter) {
        ++it;
        {  // phase 1: the wave's trip count is uniform (dist_mass is wave-cooperative)
            int i = i0, k = k0;
            for (int eb = tid - lane; eb < n; eb += nthr) {
                const int e = eb + lane;
                int jb = 0, js = 0, je = 0;  // a lane past the end: an empty run
                if (e < n) {
                    // runs as positions in the flat [N][Na] arrays (row i starts at i·Na)
                    const int* __restrict__ o = s_off + i * W;
                    const int r0 = i * Na;
                    js = o[k] + r0;
                    je = o[k + 1] + r0;
                    jb = (LOT && k > 0) ? o[k - 1] + r0 : js;
                }
                const double tot = dist_mass<LOT>(s_lam, LOT ? s_wr : nullptr, jb, js, je, 0);
                if (e < n) s_mass[e] = tot;
                k += dk;
                i += di;
                if (k >= Na) {
                    k -= Na;
                    ++i;
                }
            }
        }
        __syncthreads();
        unsigned long long key = 0ull;
        bool ok = false;
        {  // phase 2
            int m = i0, k = k0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int q = 0; q < N; ++q) acc = acc + s_P[q * N + m] * s_mass[q * Na + k];
                const double d = fabs(acc - s_lam[e]);
                s_lam[e] = acc;  // λ = λ' (this thread's own element)
                if (d == d) {
                    const unsigned long long kb = (unsigned long long)aiy_dbits(d);
                    key = kb > key ? kb : key;
                    ok = true;
                }
                k += dk;
                m += di;
                if (k >= Na) {
                    k -= Na;
                    ++m;
                }
            }
        }
        key = wave_max_u64_lane63(key);
        const unsigned lo32 = __builtin_amdgcn_readlane((int)(unsigned)key, 63);
        const unsigned hi32 = __builtin_amdgcn_readlane((int)(unsigned)(key >> 32), 63);
        const int fl = __ballot(ok) != 0ull ? 1 : 0;
        if (lane == 0) {
            s_key[wave] = ((unsigned long long)hi32 << 32) | lo32;
            s_fl[wave] = fl;
        }
        __syncthreads();
        // every thread folds the waves' entries (LDS broadcasts): the same decision in all
        unsigned long long kmax = 0ull;
        int f = 0;
        for (int v = 0; v < (nthr >> 6); ++v) {
            kmax = s_key[v] > kmax ? s_key[v] : kmax;
            f |= s_fl[v];
        }
        dist = f ? aiy_bitsd(kmax) : __builtin_nan("");
        if (dist < A.tol) break;
    }

    for (int e = tid; e < n; e += nthr) A.out[base + e] = s_lam[e];
    if (tid == 0) {
        A.iters[cand] = it;
        A.dist[cand] = dist;
    }
}

// dist_capital_kernel and fold_kernel (dist_kernels.hip) on candidate blockIdx.y / blockIdx.x
__global__ void dist_capital_batch_kernel(DistBatchArgs A) {
    __shared__ double sh[256];
    const int c = blockIdx.y;
    if (A.flags[c] != 0u) return;
    const int Na = A.Na, n = A.N * Na;
    const double* __restrict__ lam = A.out + (size_t)c * n;
    double acc = 0.0;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256)
        acc = acc + lam[t] * A.a[t % Na];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) A.part[(size_t)c * kDistCapitalBlocks + blockIdx.x] = sh[0];
}
__global__ void dist_fold_batch_kernel(DistBatchArgs A) {
    const int c = blockIdx.x;
    if (threadIdx.x != 0 || A.flags[c] != 0u) return;
    const double* __restrict__ part = A.part + (size_t)c * kDistCapitalBlocks;
    double acc = 0.0;
    for (int q = 0; q < kDistCapitalBlocks; ++q) acc = acc + part[q];
    A.k[c] = acc;
}

static int check_batch(const DistBatchArgs& A) {
    if (A.C < 1 || A.C > 65535 || !dist_batch_fits(A.N, A.Na, A.lottery))
        return fail(AIY_BAD_SHAPE, "batched histogram solve: the candidate's arrays exceed one "
                                   "CU's LDS, or more than 65,535 candidates");
    return AIY_OK;
}

int launch_dist_batch_prepare(const DistBatchArgs& A, hipStream_t st) {
    AIY_TRY(check_batch(A));
    const int n = A.N * A.Na, nw = A.N * (A.Na + 1);
    dist_batch_keys_kernel<<<dim3((n + 255) / 256, A.C), 256, 0, st>>>(A);
    dist_batch_offsets_kernel<<<dim3((nw + 255) / 256, A.C), 256, 0, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_dist_solve_batch(const DistBatchArgs& A, hipStream_t st) {
    AIY_TRY(check_batch(A));
    if (A.max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    const size_t lds = dist_batch_lds_bytes(A.N, A.Na, A.lottery);
    const int n = A.N * A.Na;
    const int nthr = std::min(1024, std::max(64, (n + 63) & ~63));
    if (A.lottery) {
        if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
            AIY_TRY((raise_dynamic_lds<dist_solve_batch_kernel<true>>((int)kDistBatchMaxLds)));
        dist_solve_batch_kernel<true><<<A.C, nthr, lds, st>>>(A);
    } else {
        if (lds > 64 * 1024)
            AIY_TRY((raise_dynamic_lds<dist_solve_batch_kernel<false>>((int)kDistBatchMaxLds)));
        dist_solve_batch_kernel<false><<<A.C, nthr, lds, st>>>(A);
    }
    if (A.k) {
        dist_capital_batch_kernel<<<dim3(kDistCapitalBlocks, A.C), 256, 0, st>>>(A);
        dist_fold_batch_kernel<<<A.C, 64, 0, st>>>(A);
    }
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
