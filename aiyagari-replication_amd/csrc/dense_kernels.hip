// Dense solve, many systems per launch (new; the reference has no linear algebra of its own).  The
// general-equilibrium step of the sequence-space method is a solve with I − M, one per economy;
// dense_solve_batch_kernel takes C of them, one workgroup per system, in dense.hpp's operation
// order.
//
// The working copy W = (A | B), [n][n+R], lives in global memory (at n = 300 it does not fit one
// CU's LDS) and is touched by its own workgroup only; LDS holds the column's multipliers l [n]
// and the waves' pivot candidates.  Column j is three phases, a barrier after each:
//   1. pivot: thread u scans rows j + u, j + u + nthr, … of column j ascending, keeping the first
//      strictly larger magnitude (a NaN never compares larger); lanes, then waves, are folded by
//      (larger magnitude, else lower row).  Row j's own entry goes to LDS as it is: a NaN there
//      ends the system, as the sequential scan would never replace it.
//   2. swap and multipliers: one thread per column k >= j exchanges rows j and p; one thread per
//      row i > j forms l_i from the column as it was before the swap (row p reads row j's entry
//      from LDS, so no thread reads a word another writes in this phase).
//   3. the trailing update, one element per thread and trip, k fastest.
// The back-substitution is one phase a step: the thread that finishes B[j−1][q] divides it by
// A[j−1][j−1] at once, so step j − 1 finds its X row ready.  Which thread does an operation
// changes nothing in it.  No workgroup waits for another: no atomics, every loop bounded by n.
#include "aiy_common.hpp"
#include "dense.hpp"

#include <algorithm>
#include <limits>

namespace aiy {

__global__ __launch_bounds__(1024) void dense_solve_batch_kernel(DenseSolveArgs A) {
    extern __shared__ __align__(16) unsigned char dense_lds[];
    __shared__ double s_pa[16], s_pv[16], s_ajj;
    __shared__ int s_pi[16];
    double* const s_l = reinterpret_cast<double*>(dense_lds);  // [n]
    const int n = A.n, R = A.R, Wp = n + R;
    const int c = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int nw = nthr >> 6;
    double* const W = A.W + (size_t)c * n * Wp;
    double* const X = A.X + (size_t)c * n * R;
    {
        const double* __restrict__ Ac = A.A + (size_t)c * n * n;
        const double* __restrict__ Bc = A.B + (size_t)c * n * R;
        int i = tid / Wp, k = tid - i * Wp;
        const int di = nthr / Wp, dk = nthr - di * Wp;
        for (int e = tid; e < n * Wp; e += nthr) {
            W[e] = k < n ? Ac[i * n + k] : Bc[i * R + (k - n)];
            k += dk;
            i += di;
            if (k >= Wp) {
                k -= Wp;
                ++i;
            }
        }
    }
    __syncthreads();

    int failed = -1;
    for (int j = 0; j < n; ++j) {
        {  // 1. the pivot of column j
            double ba = -1.0, bv = 0.0;
            int bi = n;
            for (int i = j + tid; i < n; i += nthr) {
                const double v = W[i * Wp + j], a = fabs(v);
                if (i == j) s_ajj = v;
                if (a > ba) {
                    ba = a;
                    bv = v;
                    bi = i;
                }
            }
            for (int s = 32; s > 0; s >>= 1) {
                const double oa = __shfl_down(ba, s), ov = __shfl_down(bv, s);
                const int oi = __shfl_down(bi, s);
                if (oa > ba || (oa == ba && oi < bi)) {
                    ba = oa;
                    bv = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                s_pa[wave] = ba;
                s_pv[wave] = bv;
                s_pi[wave] = bi;
            }
        }
        __syncthreads();
        // every thread folds the waves' candidates (LDS broadcasts): the same decision in all
        double best = s_pa[0], apj = s_pv[0];
        int p = s_pi[0];
        for (int v = 1; v < nw; ++v) {
            const double oa = s_pa[v];
            const int oi = s_pi[v];
            if (oa > best || (oa == best && oi < p)) {
                best = oa;
                apj = s_pv[v];
                p = oi;
            }
        }
        const double ajj = s_ajj;
        if (ajj != ajj || !(best > 0) || !(best <= std::numeric_limits<double>::max())) {
            failed = j;
            break;
        }
        // 2. rows j and p change places; l_i of the column as the swap leaves it
        if (p != j)
            for (int k = j + tid; k < Wp; k += nthr) {
                const double u = W[j * Wp + k], v = W[p * Wp + k];
                W[j * Wp + k] = v;
                W[p * Wp + k] = u;
            }
        for (int i = j + 1 + tid; i < n; i += nthr) {
            const double v = i == p ? ajj : W[i * Wp + j];
            s_l[i] = v / apj;
        }
        __syncthreads();
        {  // 3. the trailing update: rows j+1 … n−1, columns j+1 … n+R−1
            const int b = j + 1, wd = Wp - b, cnt = (n - b) * wd;
            const double* const rowj = W + j * Wp + b;
            int il = tid / wd, kl = tid - il * wd;
            const int di = nthr / wd, dk = nthr - di * wd;
            for (int e = tid; e < cnt; e += nthr) {
                double* const w = W + (b + il) * Wp + b + kl;
                *w = *w - s_l[b + il] * rowj[kl];
                kl += dk;
                il += di;
                if (kl >= wd) {
                    kl -= wd;
                    ++il;
                }
            }
        }
        __syncthreads();
    }

    if (failed >= 0) {  // (the same LDS words in every thread: the workgroup leaves together)
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int e = tid; e < n * R; e += nthr) X[e] = nan;
        if (tid == 0) {
            A.status[c] = 1;
            A.fail[c] = failed;
        }
        return;
    }

    for (int q = tid; q < R; q += nthr)
        X[(n - 1) * R + q] = W[(n - 1) * Wp + n + q] / W[(n - 1) * Wp + (n - 1)];
    __syncthreads();
    for (int j = n - 1; j >= 1; --j) {
        const double* const xj = X + j * R;
        int i = tid / R, q = tid - i * R;
        const int di = nthr / R, dq = nthr - di * R;
        for (int e = tid; e < j * R; e += nthr) {
            double* const w = W + i * Wp + n + q;
            const double bn = *w - W[i * Wp + j] * xj[q];
            *w = bn;
            if (i == j - 1) X[i * R + q] = bn / W[i * Wp + i];
            q += dq;
            i += di;
            if (q >= R) {
                q -= R;
                ++i;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        A.status[c] = 0;
        A.fail[c] = -1;
    }
}

int launch_dense_solve_batch(const DenseSolveArgs& A, hipStream_t st) {
    if (A.C < 1) return fail(AIY_BAD_SHAPE, "dense solve needs C >= 1");
    if (!dense_fits(A.n, A.R))
        return fail(AIY_BAD_SHAPE, "dense solve needs 1 <= n <= 4096, R >= 1 and n·(n + R) < 2^31");
    // a quarter of the first column's update per thread
    const size_t work = dense_work_doubles(A.n, A.R);
    const int nthr =
        (int)std::min<size_t>(1024, std::max<size_t>(64, ((work + 3) / 4 + 63) & ~(size_t)63));
    dense_solve_batch_kernel<<<A.C, nthr, sizeof(double) * (size_t)A.n, st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
