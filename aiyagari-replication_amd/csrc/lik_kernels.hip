// Second moments and the Gaussian likelihood from the sequence-space Jacobian (new; the reference
// solves stationary problems only).  The general-equilibrium Jacobians G of the observables do not
// depend on the shock process, so a candidate process costs one product and one small dense
// factorisation.
//
// ssj_ma_batch_kernel — m = dZ·Gᵀ on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), in
// ssj_fake_news_kernel's tile scheme: a workgroup of four waves owns 32 candidates x 32 rows
// (o, t) of G and walks s in chunks of 32 staged in LDS at row pitch 34.  A wave owns a 16 x 16
// quarter: A = dZ[c][s] (lane l: candidate l & 15, s = l >> 4), B = G[row][s] (lane l: s = l >> 4,
// row l & 15), C/D in the f64 layout (row l & 15, candidate (l >> 4) + 4·reg) — consecutive lanes
// store consecutive t.  Candidates past C, rows past n_o·T and s past T are zeros in LDS.  Entry
// (c, o, t) is the chain of ⌈T/4⌉ MFMA steps over s ascending, whatever the tile, C or n_o: no
// atomics, no split of s across waves or workgroups.
//
// ssj_loglik_batch_kernel — one workgroup per candidate, everything in dynamic LDS sized by this
// launch's (n_o, L, T) (lik.hpp states the arithmetic operation for operation):
//   Γ.  m [n_o][T] is staged where the triangle will be; one thread per (l, o, p) sums its lag;
//   V.  the packed lower triangle of the block-Toeplitz covariance from Γ, me_var on the diagonal;
//   LDLᵀ. right-looking and square-root free, two barriers a column: (a) w_i = V[i][j] and
//       l_i = w_i/d_j for the rows below j and for z's row; (b) the trailing update.  The triangle
//       of a column's update is folded into a rectangle — local rows p and r−1−p side by side, r+1
//       wide — so that no lane idles; which thread updates an element changes nothing in it.
//       d_j is read by every thread from LDS, so a failed pivot ends the whole workgroup at once.
//   Σ.  thread j forms aiy_log(d_j) and (z_j·z_j)/d_j; thread 0 adds them, j ascending.
// A NaN in one candidate's m reaches one of that candidate's pivots (status 1) and nothing else.
#include "aiy_common.hpp"
#include "lik.hpp"

#include <algorithm>
#include <limits>

namespace aiy {

typedef double lik_v4d __attribute__((ext_vector_type(4)));
constexpr int kMaTile = 32;             // candidates and rows of G per workgroup
constexpr int kMaChunk = 32;            // s per LDS stage
constexpr int kMaPitch = kMaChunk + 2;  // LDS row pitch (doubles), as ssj_fake_news_kernel's

__global__ __launch_bounds__(256) void ssj_ma_batch_kernel(SsjMaArgs A) {
    __shared__ double s_z[kMaTile * kMaPitch];
    __shared__ double s_g[kMaTile * kMaPitch];
    const int T = A.T, C = A.C, R = A.n_o * A.T;
    const int c0 = blockIdx.x * kMaTile, r0 = blockIdx.y * kMaTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int wc = (wave >> 1) * 16, wr = (wave & 1) * 16;
    // this thread's four (row, s) places of a stage: s = tid & 31, rows tid >> 5 + 8·u
    const int lk = tid & (kMaChunk - 1), lrow = tid >> 5;
    lik_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < T; kb += kMaChunk) {
        const int k = kb + lk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = lrow + 8 * u;
            const int c = c0 + row, r = r0 + row;
            double zv = 0.0, gv = 0.0;
            if (k < T) {
                if (c < C) zv = A.dZ[(size_t)c * T + k];
                if (r < R) gv = A.G[(size_t)r * T + k];
            }
            s_z[row * kMaPitch + lk] = zv;
            s_g[row * kMaPitch + lk] = gv;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kMaChunk; kk += 4) {
            const double av = s_z[(wc + lr) * kMaPitch + kk + lq];
            const double bv = s_g[(wr + lr) * kMaPitch + kk + lq];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int r = r0 + wr + lr;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = c0 + wc + lq + 4 * g;
        if (c < C && r < R) A.m[(size_t)c * R + r] = acc[g];
    }
}

template <bool FACTOR>
__global__ __launch_bounds__(1024) void ssj_loglik_batch_kernel(SsjLikArgs A) {
    extern __shared__ __align__(16) unsigned char lik_lds[];
    const int no = A.n_o, T = A.T, L = A.L, n = no * L;
    const int c = blockIdx.x;  // (the grid is exactly C workgroups)
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int tri = FACTOR ? n * (n + 1) / 2 : 0, mt = no * T;
    double* const s_V = reinterpret_cast<double*>(lik_lds);  // m first, then the triangle
    double* const s_G = s_V + (tri > mt ? tri : mt);         // Γ [L][n_o][n_o]
    double* const s_w = s_G + n * no;                        // [n + 1]
    double* const s_l = s_w + (n + 1);                       // [n + 1]
    double* const s_z = s_l + (n + 1);                       // [n]

    const double* __restrict__ m = A.m + (size_t)c * mt;
    for (int e = tid; e < mt; e += nthr) s_V[e] = m[e];
    __syncthreads();
    {  // Γ: one thread per (l, o, p)
        double* __restrict__ Gc = A.Gamma ? A.Gamma + (size_t)c * n * no : nullptr;
        const int noo = no * no;
        for (int e = tid; e < n * no; e += nthr) {
            const int l = e / noo, op = e - l * noo;
            const int o = op / no, p = op - o * no;
            const double* __restrict__ mo = s_V + o * T + l;
            const double* __restrict__ mp = s_V + p * T;
            double acc = 0.0;
            for (int u = 0; u < T - l; ++u) acc = acc + mo[u] * mp[u];
            s_G[e] = acc;
            if (Gc) Gc[e] = acc;
        }
    }
    if (!FACTOR) return;
    __syncthreads();
    {  // V from Γ (m is no longer needed), z = y
        const double* __restrict__ mev = A.me_var + (size_t)c * A.me_stride;
        for (int e = tid; e < n * n; e += nthr) {
            const int i = e / n, k = e - i * n;
            if (k > i) continue;
            const int t = i / no, o = i - t * no, tp = k / no, p = k - tp * no;
            double v = s_G[((t - tp) * no + o) * no + p];
            if (i == k) v = v + mev[o];
            s_V[i * (i + 1) / 2 + k] = v;
        }
        for (int k = tid; k < n; k += nthr) s_z[k] = A.y[k];
    }
    __syncthreads();

    double* __restrict__ dc = A.d ? A.d + (size_t)c * n : nullptr;
    int failed = -1;
    for (int j = 0; j < n; ++j) {
        const double dj = s_V[j * (j + 1) / 2 + j];
        if (!(dj > 0)) {  // (the same LDS word in every thread: the workgroup leaves together)
            failed = j;
            break;
        }
        // (a) the column below the pivot, and z's row as row n
        for (int i = j + 1 + tid; i <= n; i += nthr) {
            const double w = i < n ? s_V[i * (i + 1) / 2 + j] : s_z[j];
            s_w[i] = w;
            s_l[i] = w / dj;
        }
        __syncthreads();
        // (b) the trailing update: r rows, local rows p and r − 1 − p folded into one of r + 1
        const int r = n - 1 - j, W = r + 1, cnt = ((r + 1) >> 1) * W;
        const int b = j + 1;
        int p = tid / W, q = tid - p * W;
        const int dp = nthr / W, dq = nthr - dp * W;
        for (int e = tid; e < cnt; e += nthr) {
            int il, kl;
            bool ok = true;
            if (q <= p) {
                il = p;
                kl = q;
            } else {
                il = r - 1 - p;
                kl = q - (p + 1);
                ok = il != p;  // (r odd: the middle row is its own partner)
            }
            if (ok) {
                const int i = b + il, k = b + kl;
                const int a = i * (i + 1) / 2 + k;
                s_V[a] = s_V[a] - s_l[i] * s_w[k];
            }
            q += dq;
            p += dp;
            if (q >= W) {
                q -= W;
                ++p;
            }
        }
        {
            const double ln = s_l[n];
            for (int k = b + tid; k < n; k += nthr) s_z[k] = s_z[k] - ln * s_w[k];
        }
        __syncthreads();
    }

    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (failed >= 0) {
        if (dc)
            for (int k = tid; k < n; k += nthr)
                dc[k] = k <= failed ? s_V[k * (k + 1) / 2 + k] : nan;
        if (tid == 0) {
            A.loglik[c] = nan;
            A.status[c] = 1;
            A.fail[c] = failed;
        }
        return;
    }
    for (int k = tid; k < n; k += nthr) {
        const double dk = s_V[k * (k + 1) / 2 + k], zk = s_z[k];
        s_w[k] = aiy_log(dk);
        s_l[k] = (zk * zk) / dk;
        if (dc) dc[k] = dk;
    }
    __syncthreads();
    if (tid == 0) {
        double logdet = 0.0, quad = 0.0;
        for (int k = 0; k < n; ++k) logdet = logdet + s_w[k];
        for (int k = 0; k < n; ++k) quad = quad + s_l[k];
        A.loglik[c] = -0.5 * (((double)n * kLog2Pi + logdet) + quad);
        A.status[c] = 0;
        A.fail[c] = -1;
    }
}

int launch_ssj_ma_batch(const SsjMaArgs& A, hipStream_t st) {
    if (A.n_o < 1 || A.n_o > kLikMaxNo || A.T < 1 || A.T > kSsjMaxT || A.C < 1)
        return fail(AIY_BAD_SHAPE, "MA coefficients need 1 <= n_o <= 64, 1 <= T <= 32768 and "
                                   "C >= 1");
    const int R = A.n_o * A.T;  // <= 2^21: the grid's y stays below 65,536
    ssj_ma_batch_kernel<<<dim3((A.C + kMaTile - 1) / kMaTile, (R + kMaTile - 1) / kMaTile), 256, 0,
                          st>>>(A);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

int launch_ssj_loglik_batch(const SsjLikArgs& A, hipStream_t st) {
    if (A.C < 1) return fail(AIY_BAD_SHAPE, "likelihood batch needs C >= 1");
    if (!lik_fits(A.n_o, A.L, A.T))
        return fail(AIY_BAD_ARG, "likelihood batch: a candidate's arrays exceed one CU's LDS "
                                 "(lik_fits: n = L·n_o, max(n(n+1)/2, n_o·T) + n·n_o + 3n + 2 "
                                 "doubles within 160 KiB)");
    const bool factor = A.y != nullptr;
    const size_t n = (size_t)A.n_o * A.L;
    const size_t lds = lik_lds_bytes(A.n_o, A.L, A.T, factor);
    // a quarter of the first column's update, or of Γ's entries, per thread
    const size_t work = factor ? n * (n + 1) / 2 : n * (size_t)A.n_o;
    const int nthr = (int)std::min<size_t>(1024, std::max<size_t>(64, ((work + 3) / 4 + 63) & ~(size_t)63));
    if (factor) {
        if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
            AIY_TRY((raise_dynamic_lds<ssj_loglik_batch_kernel<true>>((int)kDistBatchMaxLds)));
        ssj_loglik_batch_kernel<true><<<A.C, nthr, lds, st>>>(A);
    } else {
        if (lds > 64 * 1024)
            AIY_TRY((raise_dynamic_lds<ssj_loglik_batch_kernel<false>>((int)kDistBatchMaxLds)));
        ssj_loglik_batch_kernel<false><<<A.C, nthr, lds, st>>>(A);
    }
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
