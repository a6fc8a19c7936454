// Perfect-foresight transition paths (new; the reference solves stationary problems only): the
// backward EGM pass and the forward histogram pass of C price paths, one workgroup per path.
// A path is T dependent steps whose prices change every step and whose every period policy is
// kept; through the per-step entry points that is one launch floor per step.  Path c's arrays fit
// one CU's LDS (the shapes of egm_solve_batch_kernel / dist_solve_batch_kernel), so workgroup c
// runs its T steps with no launch and no host read between them.
// No workgroup waits for another: no grid barrier, no atomics, every loop bounded by T.
//
// egm_backward_batch_kernel — LDS as egm_solve_batch_kernel<false>: policy_c [N][Na], â [N][Na],
// a_grid [Na], β(1+r[t+1])·P [N][N], w[t]·s [N], the 16 flags.  Period t = T−1 … 0:
//   0. β(1+r[t+1])·P and w[t]·s from the registers holding P and s; barrier;
//   1. per (j, a): the ordered Euler sum over m with r[t+1], c̃, â with r[t] and w[t]; barrier;
//   2. per (j, a): interp1 of the LDS row, the clamp, pk_t and pc_t to global memory, pc_t over
//      the thread's own policy_c element, the "â_j not increasing" bit; barrier; every thread
//      folds the waves' bits.
// The operations on every value are egm_fused_kernel's with r split in two, so a constant path
// reproduces T calls of aiy_egm_step_dev bit for bit.
//
// dist_forward_batch_kernel — LDS as dist_solve_batch_kernel<true>: λ, mass, lottery weights
// [N][Na] each, P, flags, run offsets [N][Na+1], and a_grid [Na].  The plan of period t is built
// in LDS inside the loop (plan choice): its keys [N][Na] (ints) and the partial
// sums of K live in the mass array, which is dead until the push.  Period t = 0 … T−1:
//   A. per (i, j): clamp pk_t, its bracket (the key) and lottery weight — dist_keys_kernel's
//      operations; the block sums of K = Σ λ_t·a in launch_dist_capital's order; barrier;
//   B. per (i, k): the run offset by binary search of the key row and the monotonicity bit —
//      dist_offsets_kernel's; thread 0 folds the block sums into K[t]; barrier; flags folded;
//   C. the push: dist_solve_batch_kernel's two phases, a barrier after each.
// pk_{t+1} is fetched into registers during period t's push.
//
// The endogenous-labour economy (A5) takes the same two passes.  labor_egm_backward_batch_kernel
// is the backward pass with egm_solve_batch_kernel<true>'s LDS (policy_c, â, c̃ [N][Na] each) and
// the labour step's operations; it also writes pl_t.  dist_forward_batch_kernel<true> is the
// forward pass plus H[t] = Σ λ_t·(s_j·pl_t): its block sums are formed beside K[t]'s in step A
// (pl_t read from global memory, s [16] in LDS after a_grid) and folded beside K[t] in step B,
// before the period's monotonicity decision.  <false> reads and writes nothing of it.
//
// Paths of several economies in one launch (aiy_ssj_jacobian_batch): with group > 0, path c
// belongs to economy c / group and reads that economy's grid, shocks, P and start array through
// strides, the backward pass also its (β, σ, amin) from a device array.  All-zero fields are the
// one-economy launch, operation for operation; the labour kernels do not read them.
#include "aiy_common.hpp"
#include "dist_dev.hpp"
#include "egm_dev.hpp"
#include "transition.hpp"

#include <algorithm>

namespace aiy {

__global__ __launch_bounds__(1024) void egm_backward_batch_kernel(EgmBackwardArgs A) {
    extern __shared__ __align__(16) unsigned char egm_back_lds[];
    const int N = A.N, Na = A.Na, n = N * Na, T = A.T;
    double* const s_c = reinterpret_cast<double*>(egm_back_lds);
    double* const s_x = s_c + n;
    double* const s_y = s_x + n;
    double* const s_P = s_y + Na;
    double* const s_ws = s_P + 256;
    int* const s_fl = reinterpret_cast<int*>(s_ws + 16 + 16);  // (after the unused 16 keys)

    const int cand = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x;  // 1,024 >= N·N
    const double* __restrict__ rc = A.r + (size_t)cand * (T + 1);
    const double* __restrict__ wc = A.w + (size_t)cand * T;
    // this path's economy (group = 0: the one economy of the launch) and its parameters
    const size_t econ = A.group > 0 ? (size_t)(cand / A.group) : 0;
    const double* __restrict__ c0 = A.pcT + (size_t)cand * A.pcT_stride + econ * A.pcT_estride;
    const double* __restrict__ a_e = A.a + econ * A.a_stride;
    const double beta = A.prm ? A.prm[3 * econ] : A.beta;
    const double sigma = A.prm ? A.prm[3 * econ + 1] : A.sigma;
    const double amin = A.prm ? A.prm[3 * econ + 2] : A.amin;
    const int ns = A.prm ? (is_int_ge(sigma, 1.0) ? (int)sigma : 0) : A.ns;
    const double p_reg = tid < N * N ? A.P[econ * A.P_stride + tid] : 0.0;
    const double s_reg = tid < N ? A.s[econ * A.s_stride + tid] : 0.0;
    for (int e = tid; e < n; e += nthr) s_c[e] = c0[e];
    for (int k = tid; k < Na; k += nthr) s_y[k] = a_e[k];

    // element e = j·Na + a of this thread's strided walk, without a division per element
    const int j0 = tid / Na, a0 = tid - j0 * Na;
    const int dj = nthr / Na, da = nthr - dj * Na;

    int status = 0, fail_t = -1;
    double r_next = rc[T], r_now = rc[T - 1], w_now = wc[T - 1];
    for (int t = T - 1; t >= 0; --t) {
        // the next period's prices, in flight during this one
        const double r_pre = t > 0 ? rc[t - 1] : 0.0, w_pre = t > 0 ? wc[t - 1] : 0.0;
        const double coef0 = beta * (1 + r_next);
        if (tid < N * N) s_P[tid] = coef0 * p_reg;
        if (tid < N) s_ws[tid] = w_now * s_reg;
        __syncthreads();
        {
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int q = 0; q < N; ++q)
                    acc = acc + s_P[j * N + q] * uprime_dev(s_c[q * Na + a_i], sigma, ns);
                const double cn = aiy_pow(acc, -1.0 / sigma);
                s_x[e] = ((cn + s_y[a_i]) - s_ws[j]) / (1 + r_now);
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        __syncthreads();
        bool bad = false;
        {
            double* __restrict__ pk_t = A.pk + ((size_t)cand * T + t) * n;
            double* __restrict__ pc_t = A.pc ? A.pc + ((size_t)cand * T + t) * n : nullptr;
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                const double* x = s_x + j * Na;
                const double q = s_y[a_i];
                double g = egm_batch_interp(x, s_y, Na, q);
                if (a_i > 0 && !(x[a_i - 1] < x[a_i])) bad = true;
                if (g < amin) g = amin;
                const double cn = ((1 + r_now) * q + s_ws[j]) - g;
                s_c[e] = cn;  // this thread's own element: the next step's pc_{t+1}
                pk_t[e] = g;
                if (pc_t) pc_t[e] = cn;
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        const int fl = __ballot(bad) != 0ull ? 1 : 0;
        if (lane == 0) s_fl[wave] = fl;
        __syncthreads();
        // every thread folds the 16 waves' bits (LDS broadcasts): the same decision in all
        int f = 0;
        for (int v = 0; v < (nthr >> 6); ++v) f |= s_fl[v];
        if (f) {  // interp1 in the reference would sort â or fail (Aiyagari_EGM.m:95)
            status = 1;
            fail_t = t;
            break;
        }
        r_next = r_now;
        r_now = r_pre;
        w_now = w_pre;
    }
    if (tid == 0) {
        A.status[cand] = status;
        A.fail_t[cand] = fail_t;
    }
}

// The labour economy's backward pass.  LDS as egm_solve_batch_kernel<true>: policy_c, â and c̃
// [N][Na] each, then β(1+r[t+1])·P, w[t]·s and the flags; a_grid is read from global memory.  The
// phases and barriers are egm_backward_batch_kernel's; the operations on every value are
// egm_fused_kernel's labour step with r split in two, so a constant path reproduces T calls of
// aiy_egm_step_dev (labor = 1) bit for bit.
__global__ __launch_bounds__(1024) void labor_egm_backward_batch_kernel(EgmBackwardArgs A) {
    extern __shared__ __align__(16) unsigned char egm_lback_lds[];
    const int N = A.N, Na = A.Na, n = N * Na, T = A.T;
    double* const s_c = reinterpret_cast<double*>(egm_lback_lds);
    double* const s_x = s_c + n;
    double* const s_y = s_x + n;
    double* const s_P = s_y + n;
    double* const s_ws = s_P + 256;
    int* const s_fl = reinterpret_cast<int*>(s_ws + 16 + 16);  // (after the unused 16 keys)

    const int cand = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x;  // 1,024 >= N·N
    const double* __restrict__ rc = A.r + (size_t)cand * (T + 1);
    const double* __restrict__ wc = A.w + (size_t)cand * T;
    const double* __restrict__ c0 = A.pcT + (size_t)cand * A.pcT_stride;
    const double p_reg = tid < N * N ? A.P[tid] : 0.0;
    const double s_reg = tid < N ? A.s[tid] : 0.0;
    for (int e = tid; e < n; e += nthr) s_c[e] = c0[e];

    // element e = j·Na + a of this thread's strided walk, without a division per element
    const int j0 = tid / Na, a0 = tid - j0 * Na;
    const int dj = nthr / Na, da = nthr - dj * Na;

    int status = 0, fail_t = -1;
    double r_next = rc[T], r_now = rc[T - 1], w_now = wc[T - 1];
    for (int t = T - 1; t >= 0; --t) {
        // the next period's prices, in flight during this one
        const double r_pre = t > 0 ? rc[t - 1] : 0.0, w_pre = t > 0 ? wc[t - 1] : 0.0;
        const double coef0 = A.beta * (1 + r_next);
        if (tid < N * N) s_P[tid] = coef0 * p_reg;
        if (tid < N) s_ws[tid] = w_now * s_reg;
        __syncthreads();
        {
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int q = 0; q < N; ++q)
                    acc = acc + s_P[j * N + q] * uprime_dev(s_c[q * Na + a_i], A.sigma, A.ns);
                const double cn = aiy_pow(acc, -1.0 / A.sigma);
                const double ws = s_ws[j];
                const double ls = labor_dev(cn, ws, A.sigma, A.ns, A.phi, A.theta);
                s_x[e] = ((cn + A.a[a_i]) - ws * ls) / (1 + r_now);
                s_y[e] = cn;
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        __syncthreads();
        bool bad = false;
        {
            const size_t o = ((size_t)cand * T + t) * n;
            double* __restrict__ pk_t = A.pk + o;
            double* __restrict__ pl_t = A.pl + o;
            double* __restrict__ pc_t = A.pc ? A.pc + o : nullptr;
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                const double* x = s_x + j * Na;
                const double q = A.a[a_i];
                double g = egm_batch_interp(x, s_y + j * Na, Na, q);
                if (a_i > 0 && !(x[a_i - 1] < x[a_i])) bad = true;
                if (q < A.amin) g = A.amin;
                const double ws = s_ws[j];
                const double l = labor_dev(g, ws, A.sigma, A.ns, A.phi, A.theta);
                const double kk = ((1 + r_now) * q + ws * l) - g;
                s_c[e] = g;  // this thread's own element: the next step's pc_{t+1}
                pk_t[e] = kk < 0 ? 0.0 : kk;
                pl_t[e] = l;
                if (pc_t) pc_t[e] = g;
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        const int fl = __ballot(bad) != 0ull ? 1 : 0;
        if (lane == 0) s_fl[wave] = fl;
        __syncthreads();
        // every thread folds the 16 waves' bits (LDS broadcasts): the same decision in all
        int f = 0;
        for (int v = 0; v < (nthr >> 6); ++v) f |= s_fl[v];
        if (f) {  // interp1 in the reference would sort â or fail
            status = 1;
            fail_t = t;
            break;
        }
        r_next = r_now;
        r_now = r_pre;
        w_now = w_pre;
    }
    if (tid == 0) {
        A.status[cand] = status;
        A.fail_t[cand] = fail_t;
    }
}

// the block sums of launch_dist_capital (dist_capital_kernel: 256 blocks of 256 threads, thread
// (b, x) the strided sum from b·256 + x, then the pairwise fold of the block) on the LDS λ: a wave
// takes a block — lane l holds the block's threads l, l + 64, l + 128, l + 192, whose fold steps
// 128 and 64 are lane-wise, steps 32 … 1 a shift down the wave.  Blocks past ⌈n/256⌉ sum to +0.
__device__ __forceinline__ void capital_parts(const double* __restrict__ lam,
                                              const double* __restrict__ a, int n, int Na,
                                              double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nb = (n + 255) >> 8;
    for (int b = wave; b < nb; b += nw) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double acc = 0.0;
            for (int t = b * 256 + u * 64 + lane; t < n; t += kDistCapitalBlocks * 256)
                acc = acc + lam[t] * a[t % Na];
            x[u] = acc;
        }
        double v = (x[0] + x[2]) + (x[1] + x[3]);
        for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s);
        if (lane == 0) part[b] = v;
    }
}
// the same block sums of H = Σ λ·(s_j·pl): the inner product rounded first
__device__ __forceinline__ void hours_parts(const double* __restrict__ lam,
                                            const double* __restrict__ pl,
                                            const double* __restrict__ s, int n, int Na,
                                            double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nb = (n + 255) >> 8;
    for (int b = wave; b < nb; b += nw) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double acc = 0.0;
            for (int t = b * 256 + u * 64 + lane; t < n; t += kDistCapitalBlocks * 256)
                acc = acc + lam[t] * (s[t / Na] * pl[t]);
            x[u] = acc;
        }
        double v = (x[0] + x[2]) + (x[1] + x[3]);
        for (int q = 32; q > 0; q >>= 1) v = v + __shfl_down(v, q);
        if (lane == 0) part[b] = v;
    }
}
// fold_kernel on those sums (one thread; the blocks past ⌈n/256⌉ add +0)
__device__ __forceinline__ double capital_fold(const double* __restrict__ part, int n) {
    double acc = 0.0;
    for (int q = 0; q < ((n + 255) >> 8); ++q) acc = acc + part[q];
    return acc;
}

constexpr int kFwdPerThread = 8;  // states per thread the pk prefetch holds

// HOURS: also H[c][t] = Σ λ_t·(s_j·pl_t) (the labour economy's effective hours); the exogenous
// instance reads and writes nothing of it.
template <bool HOURS>
__global__ __launch_bounds__(1024) void dist_forward_batch_kernel(DistForwardArgs A) {
    extern __shared__ __align__(16) unsigned char dist_fwd_lds[];
    const int N = A.N, Na = A.Na, n = N * Na, W = Na + 1, T = A.T;
    const int cand = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x;
    double* __restrict__ Kc = A.K + (size_t)cand * (T + 1);
    const double nan = __builtin_nan("");
    double* __restrict__ Hc = HOURS ? A.H + (size_t)cand * T : nullptr;
    if (A.skip && A.skip[cand] != 0) {  // workgroup-uniform: the backward pass stopped this path
        for (int t = tid; t <= T; t += nthr) Kc[t] = nan;
        if (HOURS)
            for (int t = tid; t < T; t += nthr) Hc[t] = nan;
        return;
    }
    double* const s_lam = reinterpret_cast<double*>(dist_fwd_lds);
    double* const s_mass = s_lam + n;
    double* const s_wr = s_mass + n;
    double* const s_P = s_wr + n;
    int* const s_fl = reinterpret_cast<int*>(s_P + 256 + 16);  // (after the unused 16 keys)
    int* const s_off = s_fl + 16;
    double* const s_a = reinterpret_cast<double*>(s_off + ((N * W + 1) & ~1));
    int* const s_ki = reinterpret_cast<int*>(s_mass);  // keys [N][Na]: 4n bytes of mass's 8n
    double* const s_part = s_mass + (n + 1) / 2;       // ⌈n/256⌉ <= ⌊n/2⌋ block sums of K
    double* const s_s = s_a + Na;                      // HOURS: s [16]
    // HOURS: the block sums of H after K's; n < 4 has room for one sum only: the unused key slot
    double* const s_hpart = n >= 4 ? s_part + ((n + 255) >> 8) : s_P + 256;
    const double* __restrict__ plc = HOURS ? A.pl + (size_t)cand * T * n : nullptr;

    // this path's economy (group = 0: the one economy of the launch)
    const size_t econ = A.group > 0 ? (size_t)(cand / A.group) : 0;
    const double* __restrict__ l0 = A.lam0 + (size_t)cand * A.lam0_stride + econ * A.lam0_estride;
    const double* __restrict__ pkc = A.pk + (size_t)cand * T * n;
    const double* __restrict__ P_e = A.P + econ * A.P_stride;
    const double* __restrict__ a_e = A.a + econ * A.a_stride;
    for (int q = tid; q < N * N; q += nthr) s_P[q] = P_e[q];
    for (int e = tid; e < n; e += nthr) s_lam[e] = l0[e];
    for (int k = tid; k < Na; k += nthr) s_a[k] = a_e[k];
    if (HOURS && tid < N) s_s[tid] = A.s[tid];
    double xk[kFwdPerThread];  // this thread's states of the coming period's pk
#pragma unroll
    for (int u = 0; u < kFwdPerThread; ++u) {
        const int e = tid + u * nthr;
        xk[u] = e < n ? pkc[e] : 0.0;
    }
    __syncthreads();

    // element e = i·Na + k of this thread's strided walk, without a division per element
    const int i0 = tid / Na, k0 = tid - i0 * Na;
    const int di = nthr / Na, dk = nthr - di * Na;

    int status = 0, fail_t = -1;
    int t = 0;
    for (; t < T; ++t) {
        {  // A: dist_keys_kernel on pk_t, and the block sums of K[t]
            const double a_lo = s_a[0], a_hi = s_a[Na - 1];
#pragma unroll
            for (int u = 0; u < kFwdPerThread; ++u) {
                const int e = tid + u * nthr;
                if (e < n) {
                    double x = xk[u];
                    x = x < a_lo ? a_lo : x;
                    x = x > a_hi ? a_hi : x;
                    const int key = seg_of_dev(s_a, Na, x);
                    s_wr[e] = (x - s_a[key]) / (s_a[key + 1] - s_a[key]);
                    s_ki[e] = key;
                }
            }
            capital_parts(s_lam, s_a, n, Na, s_part);
            if (HOURS) hours_parts(s_lam, plc + (size_t)t * n, s_s, n, Na, s_hpart);
        }
        __syncthreads();
        bool bad = false;
        for (int q = tid; q < N * W; q += nthr) {  // B: dist_offsets_kernel
            const int i = q / W, k = q - i * W;
            const int* __restrict__ row = s_ki + i * Na;
            if (k >= 1 && k < Na && row[k - 1] > row[k]) bad = true;
            int lo = 0, hi = Na;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (row[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            s_off[q] = lo;
        }
        const int fl = __ballot(bad) != 0ull ? 1 : 0;
        if (lane == 0) s_fl[wave] = fl;
        if (tid == 0) Kc[t] = capital_fold(s_part, n);
        if (HOURS && tid == 0) Hc[t] = capital_fold(s_hpart, n);
        __syncthreads();
        int f = 0;
        for (int v = 0; v < (nthr >> 6); ++v) f |= s_fl[v];
        if (f) {  // a non-monotone period policy: its runs are not contiguous
            status = 2;
            fail_t = t;
            break;
        }
        if (t + 1 < T) {  // the next period's policy, in flight during the push
            const double* __restrict__ pkn = pkc + (size_t)(t + 1) * n;
#pragma unroll
            for (int u = 0; u < kFwdPerThread; ++u) {
                const int e = tid + u * nthr;
                xk[u] = e < n ? pkn[e] : 0.0;
            }
        }
        {  // C, phase 1: the wave's trip count is uniform (dist_mass is wave-cooperative)
            int i = i0, k = k0;
            for (int eb = tid - lane; eb < n; eb += nthr) {
                const int e = eb + lane;
                int jb = 0, js = 0, je = 0;  // a lane past the end: an empty run
                if (e < n) {
                    const int* __restrict__ o = s_off + i * W;
                    const int r0 = i * Na;
                    js = o[k] + r0;
                    je = o[k + 1] + r0;
                    jb = k > 0 ? o[k - 1] + r0 : js;
                }
                const double tot = dist_mass<true>(s_lam, s_wr, jb, js, je, 0);
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
        {  // C, phase 2
            int m = i0, k = k0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int q = 0; q < N; ++q) acc = acc + s_P[q * N + m] * s_mass[q * Na + k];
                s_lam[e] = acc;  // λ_{t+1} (this thread's own element)
                k += dk;
                m += di;
                if (k >= Na) {
                    k -= Na;
                    ++m;
                }
            }
        }
        __syncthreads();
    }
    if (status == 0) {  // K[T] of the last λ
        capital_parts(s_lam, s_a, n, Na, s_part);
        __syncthreads();
        if (tid == 0) Kc[T] = capital_fold(s_part, n);
    } else {
        for (int q = t + 1 + tid; q <= T; q += nthr) Kc[q] = nan;
        if (HOURS)
            for (int q = t + 1 + tid; q < T; q += nthr) Hc[q] = nan;
    }
    if (A.lamT) {
        double* __restrict__ out = A.lamT + (size_t)cand * n;
        for (int e = tid; e < n; e += nthr) out[e] = s_lam[e];
    }
    if (tid == 0) {
        A.status[cand] = status;
        A.fail_t[cand] = fail_t;
    }
}

static int check_paths(int C, int T) {
    if (C < 1 || T < 1) return fail(AIY_BAD_SHAPE, "transition kernels need C >= 1 and T >= 1");
    return AIY_OK;
}

int launch_egm_backward_batch(const EgmBackwardArgs& A, hipStream_t st) {
    AIY_TRY(check_paths(A.C, A.T));
    if (!egm_backward_fits(A.N, A.Na))
        return fail(AIY_BAD_ARG, "backward EGM pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, Na <= 1024, (2N+1)·Na doubles within 160 KiB)");
    const size_t lds = egm_batch_lds_bytes(A.N, A.Na, false);
    if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
        AIY_TRY((raise_dynamic_lds<egm_backward_batch_kernel>((int)kEgmBatchMaxLds)));
    egm_backward_batch_kernel<<<A.C, 1024, lds, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_dist_forward_batch(const DistForwardArgs& A, hipStream_t st) {
    AIY_TRY(check_paths(A.C, A.T));
    const int n = A.N * A.Na;
    const int nthr = std::min(1024, std::max(64, (n + 63) & ~63));
    if (!dist_forward_fits(A.N, A.Na) || (n + nthr - 1) / nthr > kFwdPerThread)
        return fail(AIY_BAD_ARG, "forward histogram pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.2 KB within 160 KiB)");
    const size_t lds = dist_forward_lds_bytes(A.N, A.Na);
    if (lds > 64 * 1024)
        AIY_TRY((raise_dynamic_lds<dist_forward_batch_kernel<false>>((int)kDistBatchMaxLds)));
    dist_forward_batch_kernel<false><<<A.C, nthr, lds, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_labor_egm_backward_batch(const EgmBackwardArgs& A, hipStream_t st) {
    AIY_TRY(check_paths(A.C, A.T));
    if (!labor_egm_backward_fits(A.N, A.Na))
        return fail(AIY_BAD_ARG, "backward labour EGM pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, Na <= 1024, 3·N·Na doubles within 160 KiB)");
    const size_t lds = egm_batch_lds_bytes(A.N, A.Na, true);
    if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
        AIY_TRY((raise_dynamic_lds<labor_egm_backward_batch_kernel>((int)kEgmBatchMaxLds)));
    labor_egm_backward_batch_kernel<<<A.C, 1024, lds, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_labor_dist_forward_batch(const DistForwardArgs& A, hipStream_t st) {
    AIY_TRY(check_paths(A.C, A.T));
    const int n = A.N * A.Na;
    const int nthr = std::min(1024, std::max(64, (n + 63) & ~63));
    if (!labor_dist_forward_fits(A.N, A.Na) || (n + nthr - 1) / nthr > kFwdPerThread)
        return fail(AIY_BAD_ARG, "forward pass with hours: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.3 KB within 160 KiB)");
    const size_t lds = labor_dist_forward_lds_bytes(A.N, A.Na);
    if (lds > 64 * 1024)
        AIY_TRY((raise_dynamic_lds<dist_forward_batch_kernel<true>>((int)kDistBatchMaxLds)));
    dist_forward_batch_kernel<true><<<A.C, nthr, lds, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
