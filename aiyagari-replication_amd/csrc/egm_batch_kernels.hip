// A4 / A5 at many candidate rates — the whole EGM solve of one candidate in one workgroup.
//   A4: Aiyagari_EGM.m:71-110 (GE copy :177-211)
//   A5: Aiyagari_Endogenous_Labor_EGM.m:64-107 (GE copy :174-211)
// At the scripts' grid (Na = 400, N = 7) one EGM step is a launch's fixed cost, not work, and a
// solve is a chain of ~100-1000 such steps.  A candidate's chain fits one CU's LDS and the
// candidates of a GE round are independent, so workgroup c (1,024 threads) runs candidate c's
// loop from its own (r_c, w_c) and starting policy_c with no launch, no host read and no
// speculation between steps; a round of the bisection tree costs about its longest member.
// No workgroup waits for another: no grid barrier, no atomics, every loop bounded by max_iter.
//
// LDS (dynamic, 16-byte aligned base): policy_c [N][Na], â [N][Na], y (a_grid [Na] in A4, c̃
// [N][Na] in A5), then β(1+r)·P [N][N], w·s [N] and the reduction's 16 keys and flags.
// A step is two phases with one barrier after each:
//   1. per (j, a): the ordered Euler sum over m, c̃ = RHS^(-1/σ), â (and the labour FOC) — as
//      egm_fused_kernel, u'(c_m) recomputed per row (a pure function);
//   2. per (j, a): #{k : â_jk <= a_grid(a)} by binary search of the LDS row, interp1's formula,
//      the clamps, policy_c_next over the thread's own policy_c element (read first for |Δc|),
//      and the workgroup-wide max of |Δc| over finite entries + the "some finite" bit + the
//      "â_j not increasing" bit, as fold_slots_host reads egm_fused_kernel's slots.
// The operations on every value are egm_fused_kernel's, so policy_c, policy_k, policy_l, the
// iteration count and dist equal aiy_egm_solve_dev's bit for bit.  policy_k and policy_l are
// needed of the last step only: they are formed once, after the loop, from the â and y the last
// step left in LDS.
#include "aiy_common.hpp"
#include "egm.hpp"
#include "egm_dev.hpp"

namespace aiy {

template <bool LAB>
__global__ __launch_bounds__(1024) void egm_solve_batch_kernel(EgmBatchArgs A) {
    extern __shared__ __align__(16) unsigned char egm_batch_lds[];
    const int N = A.N, Na = A.Na, n = N * Na;
    double* const s_c = reinterpret_cast<double*>(egm_batch_lds);
    double* const s_x = s_c + n;
    double* const s_y = s_x + n;
    double* const s_P = s_y + (LAB ? n : Na);
    double* const s_ws = s_P + 256;
    unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(s_ws + 16);
    int* const s_fl = reinterpret_cast<int*>(s_key + 16);

    const int cand = blockIdx.x;  // (the grid is exactly C workgroups)
    const size_t base = (size_t)cand * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x;
    const double r = A.r[cand], w = A.w[cand];
    const double coef0 = A.beta * (1 + r);
    for (int q = tid; q < N * N; q += nthr) s_P[q] = coef0 * A.P[q];
    if (tid < N) s_ws[tid] = w * A.s[tid];
    for (int e = tid; e < n; e += nthr) s_c[e] = A.c[base + e];
    if (!LAB)
        for (int k = tid; k < Na; k += nthr) s_y[k] = A.a[k];
    __syncthreads();

    // element e = j·Na + a of this thread's strided walk, without a division per element
    const int j0 = tid / Na, a0 = tid - j0 * Na;
    const int dj = nthr / Na, da = nthr - dj * Na;

    long long it = 0;
    double dist = 1.0;  // :72 — tested before the first step
    int status = 0;
    while (dist > A.tol && it < A.max_iter) {  // :74
        ++it;
        {  // :80-92 (labour :80-87)
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                double acc = 0.0;
                for (int q = 0; q < N; ++q)
                    acc = acc + s_P[j * N + q] * uprime_dev(s_c[q * Na + a_i], A.sigma, A.ns);
                const double cn = aiy_pow(acc, -1.0 / A.sigma);
                const double ag = LAB ? A.a[a_i] : s_y[a_i];
                const double ws = s_ws[j];
                double ah;
                if (LAB) {
                    const double ls = labor_dev(cn, ws, A.sigma, A.ns, A.phi, A.theta);
                    ah = ((cn + ag) - ws * ls) / (1 + r);
                    s_y[e] = cn;
                } else {
                    ah = ((cn + ag) - ws) / (1 + r);
                }
                s_x[e] = ah;
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        __syncthreads();
        unsigned long long key = 0ull;
        bool ok = false, bad = false;
        {  // :93-106 (labour :88-104)
            int j = j0, a_i = a0;
            for (int e = tid; e < n; e += nthr) {
                const double* x = s_x + j * Na;
                const double q = LAB ? A.a[a_i] : s_y[a_i];
                double g = egm_batch_interp(x, LAB ? s_y + j * Na : s_y, Na, q);
                if (a_i > 0 && !(x[a_i - 1] < x[a_i])) bad = true;
                double cn;
                if (LAB) {
                    if (q < A.amin) g = A.amin;
                    cn = g;
                } else {
                    if (g < A.amin) g = A.amin;
                    cn = ((1 + r) * q + s_ws[j]) - g;
                }
                const double d = fabs(cn - s_c[e]);
                s_c[e] = cn;  // :107 policy_c = policy_c_next (this thread's own element)
                if (d == d) {
                    const unsigned long long kb = (unsigned long long)aiy_dbits(d);
                    key = kb > key ? kb : key;
                    ok = true;
                }
                a_i += da;
                j += dj;
                if (a_i >= Na) {
                    a_i -= Na;
                    ++j;
                }
            }
        }
        key = wave_max_u64_lane63(key);
        const unsigned lo32 = __builtin_amdgcn_readlane((int)(unsigned)key, 63);
        const unsigned hi32 = __builtin_amdgcn_readlane((int)(unsigned)(key >> 32), 63);
        const int fl = (__ballot(ok) != 0ull ? 1 : 0) | (__ballot(bad) != 0ull ? 2 : 0);
        if (lane == 0) {
            s_key[wave] = ((unsigned long long)hi32 << 32) | lo32;
            s_fl[wave] = fl;
        }
        __syncthreads();
        // every thread folds the 16 waves' entries (LDS broadcasts): the same decision in all
        unsigned long long k = 0ull;
        int f = 0;
        for (int v = 0; v < (nthr >> 6); ++v) {
            k = s_key[v] > k ? s_key[v] : k;
            f |= s_fl[v];
        }
        dist = (f & 1) ? aiy_bitsd(k) : __builtin_nan("");
        if (f & 2) {  // interp1 in the reference would sort â or fail (Aiyagari_EGM.m:95)
            status = 1;
            break;
        }
    }

    if (it > 0) {  // the last step's outputs from the â and y it left in LDS
        int j = j0, a_i = a0;
        for (int e = tid; e < n; e += nthr) {
            const double q = LAB ? A.a[a_i] : s_y[a_i];
            double g = egm_batch_interp(s_x + j * Na, LAB ? s_y + j * Na : s_y, Na, q);
            const double ws = s_ws[j];
            if (LAB) {
                if (q < A.amin) g = A.amin;  // :91
                const double l = labor_dev(g, ws, A.sigma, A.ns, A.phi, A.theta);  // :95
                const double kk = ((1 + r) * q + ws * l) - g;                        // :98
                A.pk[base + e] = kk < 0 ? 0.0 : kk;                                  // :99
                if (A.pl) A.pl[base + e] = l;
            } else {
                if (g < A.amin) g = A.amin;  // :98
                A.pk[base + e] = g;
            }
            A.c[base + e] = s_c[e];
            a_i += da;
            j += dj;
            if (a_i >= Na) {
                a_i -= Na;
                ++j;
            }
        }
    }
    if (tid == 0) {
        A.iters[cand] = it;
        A.dist[cand] = dist;
        A.status[cand] = status;
    }
}

int launch_egm_solve_batch(const EgmBatchArgs& A, hipStream_t st) {
    if (A.N > 16) return fail(AIY_BAD_SHAPE, "EGM kernels support N <= 16 productivity states");
    if (A.C < 1 || !egm_batch_fits(A.N, A.Na, A.labor))
        return fail(AIY_BAD_SHAPE, "batched EGM solve: the candidate's arrays exceed one CU's LDS");
    const size_t lds = egm_batch_lds_bytes(A.N, A.Na, A.labor);
    if (A.labor) {
        if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
            AIY_TRY((raise_dynamic_lds<egm_solve_batch_kernel<true>>((int)kEgmBatchMaxLds)));
        egm_solve_batch_kernel<true><<<A.C, 1024, lds, st>>>(A);
    } else {
        if (lds > 64 * 1024)
            AIY_TRY((raise_dynamic_lds<egm_solve_batch_kernel<false>>((int)kEgmBatchMaxLds)));
        egm_solve_batch_kernel<false><<<A.C, 1024, lds, st>>>(A);
    }
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
