// A8 entry point (Krusell_Smith_EGM.m:129-209): k_opt is k x K x S column-major exactly as
// in the script; P is MATLAB's 4 x 4; params = the 13-double KS block {beta, alpha, delta,
// k_min, k_max, ug, ub, l_bar, mu, z_grid(1:2), eps_grid(1:2)} (mu unused by the EGM script).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "ks_egm.hpp"
#include "ws.hpp"

#include <algorithm>

namespace aiy {

// per-pair scalars in the script's order with libm (:101-112 tables, :139-175)
static void ks_egm_pairs(const double* prm, const double* K_grid, const double* B, int nK,
                         std::vector<KsEgmPair>& out) {
    const double alpha = prm[1], delta = prm[2], ug = prm[5], ub = prm[6], lb = prm[7];
    const double zg[2] = {prm[9], prm[10]}, eg[2] = {prm[11], prm[12]};
    out.resize(4 * nK);
    auto labour = [&](double z) {
        return lb * (1 - ug * (double)(z == zg[0]) - ub * (double)(z == zg[1]));
    };
    auto alm = [&](double z, double K) {
        return (z == zg[0]) ? exp(B[0] + B[1] * log(K)) : exp(B[2] + B[3] * log(K));
    };
    for (int s_i = 0; s_i < 4; ++s_i) {
        const double z = zg[s_i < 2 ? 0 : 1], e = eg[s_i % 2];  // s_grid = [Z(:), Eps(:)] (:18-19)
        for (int K_i = 0; K_i < nK; ++K_i) {
            KsEgmPair q{};
            const double K = K_grid[K_i];
            const double L = labour(z);
            const double r = alpha * z * pow(K, alpha - 1) * pow(L, 1 - alpha);  // r_table (:110)
            const double w = (1 - alpha) * z * pow(K, alpha) * pow(L, -alpha);   // w_table (:109)
            const double Kp = alm(z, K);                                         // :140-145
            for (int s_j = 0; s_j < 4; ++s_j) {
                const double zn = zg[s_j < 2 ? 0 : 1], en = eg[s_j % 2];
                const double Kd = alm(zn, Kp);                                   // :164-169
                int idx = 0;
                double bd = fabs(K_grid[0] - Kd);
                for (int m = 1; m < nK; ++m) {  // min(abs(K_grid - K_dprime)): first on ties
                    const double dd = fabs(K_grid[m] - Kd);
                    if (dd < bd) {
                        bd = dd;
                        idx = m;
                    }
                }
                const double Ln = labour(zn);
                const double rn = alpha * zn * pow(Kd, alpha - 1) * pow(Ln, 1 - alpha);  // :174
                const double wn = (1 - alpha) * zn * pow(Kd, alpha) * pow(Ln, -alpha);   // :175
                q.kd[s_j] = idx;
                q.Rn[s_j] = (1 + rn) - delta;
                q.Wn[s_j] = (wn * en) * lb;
            }
            q.R = (1 + r) - delta;
            q.We = (w * e) * lb;
            out[s_i * nK + K_i] = q;
        }
    }
}

void p_rows(const double* P, double out[16]) {
    for (int i = 0; i < 4; ++i)
        for (int m = 0; m < 4; ++m) out[i * 4 + m] = P[i + m * 4];
}

// the pair tables take log(K) and K^(alpha - 1); cand > 0 (the batch tiers) names the candidate
static int check_K_grid_positive(const double* K_grid, int64_t nK, int64_t cand = 0) {
    for (int64_t q = 0; q < nK; ++q)
        if (!(K_grid[q] > 0) || !std::isfinite(K_grid[q]))
            return cand ? fail(AIY_NON_FINITE, "K_grid must be positive and finite (candidate %lld)",
                               (long long)cand)
                        : fail(AIY_NON_FINITE, "K_grid must be positive and finite");
    return AIY_OK;
}

static int no_egm_points() {
    return fail(AIY_NON_FINITE, "an (s, K) pair had fewer than 2 valid EGM points "
                                "(griddedInterpolant needs two; Krusell_Smith_EGM.m:196)");
}

// What ks_egm_solve and ks_egm_solve_jacobi stage alike, behind their own checks.  The host
// copies live here until the caller's next wait on the stream.
struct EgmStage {
    std::vector<KsEgmPair> pairs;
    double Pr[16];
    KsEgmArgs A{};
    double* dk = nullptr;  // the policy buffer, holding k_opt in its first k x K x S block
};
// k_grid, P as rows, k_opt and the pair table up, into the buffers <pre>kg, <pre>P, `pol_name`
// (room for `slots` policies: the Jacobi ring, whose slot 0 is the start) and <pre>pairs.
static int egm_stage(HostCtx* c, const std::string& pre, const char* pol_name, size_t slots,
                     const double* k_opt, const double* k_grid, const double* K_grid,
                     const double* B, const double* P, const double* params, int64_t nk,
                     int64_t nK, double tol, int64_t max_iter, EgmStage& S) {
    ks_egm_pairs(params, K_grid, B, (int)nK, S.pairs);
    p_rows(P, S.Pr);
    const size_t n = (size_t)nk * nK * 4;
    double *dkg, *dP;
    KsEgmPair* dpairs;
    AIY_TRY(c->up((pre + "kg").c_str(), k_grid, nk, &dkg));
    AIY_TRY(c->up((pre + "P").c_str(), S.Pr, 16, &dP));
    AIY_TRY(c->room(pol_name, slots * n, &S.dk));
    AIY_TRY(c->up(pol_name, k_opt, n, &S.dk));  // (fits: the same memory)
    AIY_TRY(c->up((pre + "pairs").c_str(), S.pairs.data(), S.pairs.size(), &dpairs));
    S.A.nk = (int)nk;
    S.A.nK = (int)nK;
    S.A.max_iter = (int)max_iter;
    S.A.k_grid = dkg;
    S.A.P = dP;
    S.A.pairs = dpairs;
    S.A.beta = params[0];
    S.A.k_min = params[3];
    S.A.k_max = params[4];
    S.A.tol = tol;
    return AIY_OK;
}

// ---- the batched solve: C economies, one workgroup each (ks_egm_solve_batch_kernel)

// what both tiers check on their host arguments, before any device work
static int check_egm_batch(int64_t C, const double* K_grid, int64_t nk, int64_t nK,
                           int64_t max_iter) {
    if (C < 1 || C > kEgmBatchMaxCand) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 65,535 candidates");
    if (nk < 3 || nK < 1 || nk > (1 << 20))
        return fail(AIY_BAD_SHAPE, "need k_size >= 3 and K_size >= 1");
    if (max_iter < 1 || max_iter > 2147483647) return fail(AIY_BAD_ARG, "max_iter in [1, 2^31)");
    if (!ks_egm_fits((int)nk, (int)nK))
        return fail(AIY_BAD_SHAPE, "k_size x K_size too large for the one-workgroup EGM solve");
    for (int64_t c = 0; c < C; ++c) AIY_TRY(check_K_grid_positive(K_grid + c * nK, nK, c + 1));
    return AIY_OK;
}

// device scratch of one call: the candidates' KsEgmCand blocks, then their pair tables
static size_t egm_batch_scratch(int64_t C, int64_t nK) {
    return (size_t)C * (sizeof(KsEgmCand) + 4 * (size_t)nK * sizeof(KsEgmPair));
}

// Builds the candidates' tables on the host (libm, as ks_egm_pairs), uploads them into `scratch`
// and enqueues the one launch.  The upload is ordered on `st` behind whatever still reads
// `scratch`, and the call waits for it before the host table dies; the solve itself is left
// running on `st`.
static int egm_batch_dev(int64_t C, double* k_opt, const double* k_grid, const double* K_grid,
                         const double* B, const double* P, const double* params, int64_t nk,
                         int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff,
                         int32_t* status, void* scratch, hipStream_t st) {
    std::vector<KsEgmCand> cand(C);
    std::vector<KsEgmPair> pairs((size_t)C * 4 * nK), one;
    for (int64_t c = 0; c < C; ++c) {
        const double* prm = params + 13 * c;
        ks_egm_pairs(prm, K_grid + c * nK, B + 4 * c, (int)nK, one);
        std::copy(one.begin(), one.end(), pairs.begin() + (size_t)c * 4 * nK);
        p_rows(P + 16 * c, cand[c].P);
        cand[c].beta = prm[0];
        cand[c].k_min = prm[3];
        cand[c].k_max = prm[4];
    }
    KsEgmCand* dcand = (KsEgmCand*)scratch;
    KsEgmPair* dpairs = (KsEgmPair*)(dcand + C);
    AIY_HIP(hipMemcpyAsync(dcand, cand.data(), cand.size() * sizeof(KsEgmCand),
                           hipMemcpyHostToDevice, st));
    AIY_HIP(hipMemcpyAsync(dpairs, pairs.data(), pairs.size() * sizeof(KsEgmPair),
                           hipMemcpyHostToDevice, st));
    AIY_HIP(hipStreamSynchronize(st));
    KsEgmBatchArgs A{};
    A.nk = (int)nk;
    A.nK = (int)nK;
    A.max_iter = (int)max_iter;
    A.C = (int)C;
    A.k_grid = k_grid;
    A.cand = dcand;
    A.pairs = dpairs;
    A.tol = tol;
    A.k_opt = k_opt;
    A.iters = iters;
    A.diff = diff;
    A.status = status;
    return launch_ks_egm_solve_batch(A, st);
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int64_t ks_egm_batch_scratch_bytes(int64_t C, int64_t nK) {
    return (C < 1 || nK < 1) ? 0 : (int64_t)egm_batch_scratch(C, nK);
}

int ks_egm_solve_batch_dev(int64_t C, double* k_opt, const double* k_grid, const double* K_grid,
                           const double* B, const double* P, const double* params, int64_t nk,
                           int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff,
                           int32_t* status, void* scratch, void* stream) {
    if (!k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !diff || !status ||
        !scratch)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_egm_batch(C, K_grid, nk, nK, max_iter));
    return egm_batch_dev(C, k_opt, k_grid, K_grid, B, P, params, nk, nK, tol, max_iter, iters,
                         diff, status, scratch, (hipStream_t)stream);
}

int ks_egm_solve_batch(int64_t C, double* k_opt, const double* k_grid, const double* K_grid,
                       const double* B, const double* P, const double* params, int64_t nk,
                       int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff,
                       int32_t* status) {
    if (!k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !diff || !status)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_egm_batch(C, K_grid, nk, nK, max_iter));
    AIY_TRY(check_grid_strict(k_grid, nk));  // pchip divides by k(i+1) - k(i)
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(4 * nK, nk, 1, &c));
    const size_t n = (size_t)C * nk * nK * 4;
    double *dkg, *dk, *ddiff;
    int64_t* dit;
    int32_t* dst;
    unsigned char* dscr;
    AIY_TRY(c->up("egmb_kg", k_grid, nk, &dkg));
    AIY_TRY(c->up("egmb_k", k_opt, n, &dk));
    AIY_TRY(c->room("egmb_iters", C, &dit));
    AIY_TRY(c->room("egmb_diff", C, &ddiff));
    AIY_TRY(c->room("egmb_status", C, &dst));
    AIY_TRY(c->room("egmb_scratch", egm_batch_scratch(C, nK), &dscr));
    AIY_TRY(egm_batch_dev(C, dk, dkg, K_grid, B, P, params, nk, nK, tol, max_iter, dit, ddiff, dst,
                          dscr, c->st));
    AIY_TRY(c->down(iters, dit, C));
    AIY_TRY(c->down(diff, ddiff, C));
    AIY_TRY(c->down(status, dst, C));
    AIY_TRY(c->down(k_opt, dk, n));
    AIY_HIP(hipStreamSynchronize(c->st));
    return AIY_OK;
}

int ks_egm_solve(double* k_opt, const double* k_grid, const double* K_grid, const double* B,
                 const double* P, const double* params, int64_t nk, int64_t nK, double tol,
                 int64_t max_iter, int64_t* iters, double* diff) {
    if (!k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !diff)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (nk < 3 || nK < 1 || nk > (1 << 20))
        return fail(AIY_BAD_SHAPE, "need k_size >= 3 and K_size >= 1");
    if (max_iter < 1 || max_iter > 2147483647) return fail(AIY_BAD_ARG, "max_iter in [1, 2^31)");
    if (!ks_egm_fits((int)nk, (int)nK))
        return fail(AIY_BAD_SHAPE, "k_size x K_size too large for the one-workgroup EGM solve");
    AIY_TRY(check_grid_strict(k_grid, nk));  // pchip divides by k(i+1) - k(i)
    AIY_TRY(check_K_grid_positive(K_grid, nK));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(4 * nK, nk, 1, &c));
    EgmStage S;
    AIY_TRY(egm_stage(c, "egm_", "egm_k", 1, k_opt, k_grid, K_grid, B, P, params, nk, nK, tol,
                      max_iter, S));
    KsEgmOut* dout;
    AIY_TRY(c->room("egm_out", 1, &dout));
    AIY_TRY(launch_ks_egm_solve(S.A, S.dk, dout, c->st));
    KsEgmOut o;
    AIY_TRY(c->down(&o, dout, 1));
    AIY_TRY(c->down(k_opt, S.dk, (size_t)nk * nK * 4));
    AIY_HIP(hipStreamSynchronize(c->st));
    *iters = o.iters;
    *diff = o.diff;
    return o.status ? no_egm_points() : AIY_OK;
}

// F1 — the Jacobi variant of the KS EGM iteration: every (s, K) pair of a sweep reads the
// previous sweep's k_opt, all pairs of a sweep in one launch.  NOT the reference's result (the
// script is Gauss-Seidel, Krusell_Smith_EGM.m:199); same stop rule (:204-207).  Sweeps are
// enqueued in batches with one diff-slot set each and read back once per batch.
int ks_egm_solve_jacobi(double* k_opt, const double* k_grid, const double* K_grid,
                        const double* B, const double* P, const double* params, int64_t nk,
                        int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff) {
    if (!k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !diff)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (nk < 3 || nK < 1) return fail(AIY_BAD_SHAPE, "need k_size >= 3 and K_size >= 1");
    if (ks_egm_jacobi_lds_bytes((int)nk) > 150 * 1024)
        return fail(AIY_BAD_SHAPE, "k_size too large for one workgroup per (s, K) pair");
    if (max_iter < 1 || max_iter > 2147483647) return fail(AIY_BAD_ARG, "max_iter in [1, 2^31)");
    AIY_TRY(check_grid_strict(k_grid, nk));  // pchip divides by k(i+1) - k(i)
    AIY_TRY(check_K_grid_positive(K_grid, nK));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(4 * nK, nk, 1, &c));
    const size_t n = (size_t)nk * nK * 4;
    constexpr int kBatch = 16;
    // ring of kBatch + 1 policy buffers: sweep g reads slot (g-1) % R and writes slot g % R, so
    // the sweeps a batch runs past the stopping sweep never overwrite its output
    constexpr int R = kBatch + 1;
    EgmStage S;
    AIY_TRY(egm_stage(c, "egmj_", "egmj_ring", R, k_opt, k_grid, K_grid, B, P, params, nk, nK,
                      tol, max_iter, S));
    const KsEgmArgs& A = S.A;
    double* const ring = S.dk;
    unsigned long long* dslots;
    int* dstatus;
    AIY_TRY(c->room("egmj_slots", kBatch * 2 * kDiffSlots, &dslots));
    AIY_TRY(c->room("egmj_status", 1, &dstatus));
    AIY_HIP(hipMemsetAsync(dstatus, 0, sizeof(int), c->st));
    auto slot = [&](int64_t g) { return ring + (size_t)(g % R) * n; };
    std::vector<unsigned long long> hs(kBatch * 2 * kDiffSlots);
    int64_t done = 0, stop = 0;
    double d_last = NAN;
    int status = 0;
    while (!stop && done < max_iter) {
        const int64_t m = std::min<int64_t>(kBatch, max_iter - done);
        AIY_HIP(hipMemsetAsync(dslots, 0, m * 2 * kDiffSlots * sizeof(unsigned long long), c->st));
        for (int64_t t = 0; t < m; ++t) {
            const int64_t g = done + 1 + t;
            AIY_TRY(launch_ks_egm_jacobi(A, slot(g - 1), slot(g),
                                         dslots + t * 2 * kDiffSlots, dstatus, c->st));
        }
        AIY_TRY(c->down(hs.data(), dslots, m * 2 * kDiffSlots));
        AIY_TRY(c->down(&status, dstatus, 1));
        AIY_HIP(hipStreamSynchronize(c->st));
        if (status) break;
        for (int64_t t = 0; t < m; ++t) {
            d_last = fold_slots_host(hs.data() + t * 2 * kDiffSlots);
            if (d_last < tol) {
                stop = done + 1 + t;
                break;
            }
        }
        if (!stop) done += m;
    }
    if (status) return no_egm_points();
    const int64_t g = stop ? stop : max_iter;
    AIY_TRY(c->down(k_opt, slot(g), n));
    AIY_HIP(hipStreamSynchronize(c->st));
    *iters = g;
    *diff = d_last;
    return AIY_OK;
}

}  // extern "C"
