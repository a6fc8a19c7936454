// Config 4 host tier (BASELINE configs[3], SURVEY §8(b) B2 `ge_batch`): excess demand at C
// candidate interest rates in one call — for each candidate the body of one GE step of
// Aiyagari_VFI.m:147-195 (VFI from a common v_old, Monte-Carlo capital supply with the
// candidate's own block of MATLAB's rand stream, K_d = labor·(α/(r+δ))^(1/(1−α))).  The
// candidates are spread over n_devices GPUs of this process, each device solving its share as
// one batched solve (aiy_vfi_solve_batch_dev) and one batched launch of the chains.  The bracket
// logic stays with the caller (the MATLAB script or ge_batch.py), exactly as in the reference.
// aiy_egm_ge_batch is the same for the EGM scripts (Aiyagari_EGM.m:177-242, labour :174-240):
// the batched EGM solve (aiy_egm_solve_batch_dev) from a common policy_c with the caller's w per
// candidate; the device split, the uniforms and the chains are shared with aiy_ge_batch.
// aiy_ge_hist_batch and aiy_egm_ge_hist_batch replace the chains by the stationary histogram (A10)
// of every candidate's policy in one batched solve (aiy_dist_stationary_batch_dev).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "sim.hpp"
#include "ws.hpp"

namespace aiy {

namespace {
struct GeShare {
    int dev = 0;
    int64_t c0 = 0, cn = 0;  // candidates [c0, c0 + cn)
    HostCtx* ctx = nullptr;
    int rc = AIY_OK;
    std::string err;
};

// Splits C candidates over up to n_devices GPUs of this process (contiguous shares, the first
// C % nd one larger; share d on device (current + d) % visible) and runs body(share) on each,
// one host thread per device when there are several.  Holds the host-tier lock; the first
// failing share's status and message are the call's.
template <class Body>
int ge_run_shares(int64_t C, int64_t N, int64_t Na, int64_t Nl, int n_devices, Body body) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AIY_NO_DEVICE, "no HIP device visible");
    const int nd = (int)std::min<int64_t>(std::max(n_devices, 1), std::min<int64_t>(ndev, C));
    std::lock_guard<std::mutex> lk(host_mutex());
    int cur = 0;
    (void)hipGetDevice(&cur);
    std::vector<GeShare> sh(nd);
    for (int d = 0; d < nd; ++d) {
        sh[d].dev = (cur + d) % ndev;
        sh[d].c0 = d * (C / nd) + std::min<int64_t>(d, C % nd);
        sh[d].cn = C / nd + (d < C % nd ? 1 : 0);
        (void)hipSetDevice(sh[d].dev);
        int rc = get_ctx(N, Na, Nl, &sh[d].ctx);
        if (rc != AIY_OK) {
            (void)hipSetDevice(cur);
            return rc;
        }
    }
    auto run = [&](GeShare& g) {
        g.rc = body(g);
        if (g.rc != AIY_OK) g.err = aiy_last_error();
    };
    if (nd == 1) {
        run(sh[0]);
    } else {  // one host thread per device: the shares run concurrently
        std::vector<std::thread> th;
        for (auto& g : sh) th.emplace_back(run, std::ref(g));
        for (auto& t : th) t.join();
    }
    (void)hipSetDevice(cur);
    for (auto& g : sh)
        if (g.rc != AIY_OK) return fail(g.rc, "%s", g.err.c_str());
    return AIY_OK;
}

// w at the candidate rates of the share (Aiyagari_VFI.m:149, Aiyagari_Endogenous_Labor_VFI.m:173)
std::vector<double> ge_wages(const GeShare& sh, const double* r, double alpha, double delta) {
    std::vector<double> w(sh.cn);
    for (int64_t q = 0; q < sh.cn; ++q)
        w[q] = (1 - alpha) * std::pow(alpha / (r[sh.c0 + q] + delta), alpha / (1 - alpha));
    return w;
}

// K_d at every candidate rate (Aiyagari_VFI.m:195, Aiyagari_EGM.m:242, labour VFI :239)
void ge_demand(const double* r, int64_t C, double labor, double alpha, double delta,
               double* k_demand) {
    for (int64_t q = 0; q < C; ++q)
        k_demand[q] = labor * std::pow(alpha / (r[q] + delta), 1 / (1 - alpha));
}

int ge_check_rates(const double* r, int64_t C, double delta) {
    for (int64_t q = 0; q < C; ++q)
        if (!std::isfinite(r[q]) || r[q] + delta <= 0)
            return fail(AIY_BAD_ARG, "candidate %lld: r must be finite with r + delta > 0", (long long)q + 1);
    return AIY_OK;
}

// the chains' scalars, in the order the three Monte-Carlo entries test them
int ge_check_chain(int64_t T, int64_t z1, int64_t N, int64_t max_iter) {
    if (T < 1 || T > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "T must be in [1, 2^31)");
    if (z1 < 1 || z1 > N) return fail(AIY_BAD_ARG, "z1 (1-based) out of range");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    return AIY_OK;
}

// the two iteration limits, in the order the two histogram entries test them
int ge_check_hist(int64_t max_iter, int64_t dist_max_iter) {
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    if (dist_max_iter < 1) return fail(AIY_BAD_ARG, "dist_max_iter must be >= 1");
    return AIY_OK;
}

// run(q0, q1) for every maximal run [q0, q1) of the share's candidates with skip[q] == 0 (skip
// nullable: one run of all of them)
template <class Run>
int ge_runs(int64_t C, const int32_t* skip, Run run) {
    for (int64_t q0 = 0; q0 < C;) {
        if (skip && skip[q0]) {
            ++q0;
            continue;
        }
        int64_t q1 = q0;
        while (q1 < C && !(skip && skip[q1])) ++q1;
        AIY_TRY(run(q0, q1));
        q0 = q1;
    }
    return AIY_OK;
}

// the share's uniforms (column c of the (T-1) x C matrix = candidate c's draws) to its device
int ge_stage_uniforms(GeShare& sh, int64_t T, const double* uniforms, double** dU) {
    if (T > 1) return sh.ctx->up("ge_U", uniforms + sh.c0 * (T - 1), (size_t)((T - 1) * sh.cn), dU);
    return sh.ctx->room("ge_U", (size_t)sh.cn, dU);
}

// The share's batched chains over pk [cn][N][Na]: one batched launch per run of candidates
// with skip[q] == 0 (skip nullable: all of them in one), then K_s and the find() flags back
// (synchronises).  k_supply[c0 + q] is written for the candidates that ran; find_empty[q] for all.
int ge_chains(GeShare& sh, const double* pk, const double* da, const double* dP, const double* dU,
              int64_t N, int64_t Na, int64_t z1, double k1, int64_t T, const int32_t* skip,
              double* k_supply, int* find_empty) {
    HostCtx* c = sh.ctx;
    const int64_t C = sh.cn;
    const size_t n = (size_t)N * Na;
    double* dout;
    int* dst;
    AIY_TRY(c->room("ge_out", (size_t)C, &dout));
    AIY_TRY(c->room("ge_st", (size_t)C, &dst));
    SimArgs S{};
    S.N = (int)N; S.Na = (int)Na; S.T = (int)T; S.z1 = (int)(z1 - 1); S.k1 = k1;
    S.zs = (size_t)Na; S.as = 1; S.a = da; S.P = dP;
    S.pcs = n; S.ucs = (size_t)std::max<int64_t>(T - 1, 0);
    S.par = c->ws->sim_par;
    if (S.par != 0)  // the speculative-segment chains' scratch (paths, state paths, flags)
        AIY_TRY(c->room("ge_kscr", (sim_par_scratch_bytes(T, C) + sizeof(double) - 1) / sizeof(double),
                        &S.kscr));
    for (int64_t q = 0; q < C; ++q) find_empty[q] = 0;
    AIY_TRY(ge_runs(C, skip, [&](int64_t q0, int64_t q1) -> int {
        S.pol = pk + q0 * n;
        S.U = dU + q0 * S.ucs;
        S.out = dout + q0;
        S.status = dst + q0;
        S.C = (int)(q1 - q0);
        AIY_TRY(launch_sim_capital(S, c->st));
        // a run's results land at its offset in the caller's arrays
        AIY_TRY(c->down(k_supply + sh.c0 + q0, dout + q0, (size_t)(q1 - q0)));
        return c->down(find_empty + q0, dst + q0, (size_t)(q1 - q0));
    }));
    return c->sync();
}

// the chains' find(rand < cumsum(P(z,:))) came up empty somewhere: the VFI entries' failure
int ge_find_empty(const GeShare& sh, const std::vector<int>& status) {
    for (int64_t q = 0; q < sh.cn; ++q)
        if (status[q]) return fail(AIY_FIND_EMPTY, "candidate %lld: find(rand < cumsum(P(z,:))) empty",
                                   (long long)(sh.c0 + q + 1));
    return AIY_OK;
}

// what a share's solve leaves on its device for the supply step
struct GeSolved {
    double *da = nullptr, *dP = nullptr, *pk = nullptr;  // a_grid, P rows, policy_k [cn][N][Na]
    int* idx = nullptr;                                  // VFI: the index policy, 0-based
};

// VFI stage + batched solve of one share: every candidate from the same v_old (the caller's
// warm start, v_rows [N][Na]) at its own wage
int ge_vfi_solve(GeShare& sh, const double* r, const double* v_rows, const double* a,
                 const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                 double delta, double beta, double sigma, double tol, int64_t max_iter,
                 int64_t* iters, GeSolved* g) {
    HostCtx* c = sh.ctx;
    const int64_t C = sh.cn;
    const size_t n = (size_t)N * Na;
    double *ds, *va, *vb;
    AIY_TRY(stage_common(c, a, s, P, N, Na, &g->da, &ds, &g->dP));
    AIY_TRY(c->bcast("ge_va", v_rows, n, C, &va));
    AIY_TRY(c->room("ge_vb", n * C, &vb));
    AIY_TRY(c->room("ge_pk", n * C, &g->pk));
    AIY_TRY(c->room("ge_idx", n * C, &g->idx));
    const std::vector<double> w = ge_wages(sh, r, alpha, delta);
    std::vector<int> which(C);
    return bell_solve_batch_dev(c->ws, C, r + sh.c0, w.data(), va, vb, g->da, ds, g->dP, beta,
                                sigma, tol, max_iter, 0, g->idx, g->pk, nullptr, iters + sh.c0,
                                which.data(), c->st);
}

// EGM stage + batched solve of one share: every candidate from the same policy_c (Na x N
// column-major == [N][Na]) at the caller's w; status[c0 + q] != 0 where a candidate failed
int ge_egm_solve(GeShare& sh, const double* r, const double* w, const double* pc_start,
                 const double* a, const double* s, const double* P, int64_t N, int64_t Na,
                 double beta, double sigma, double amin, int labor, double phi, double theta,
                 double tol, int64_t max_iter, int64_t* iters, int32_t* status, GeSolved* g) {
    HostCtx* c = sh.ctx;
    const int64_t C = sh.cn;
    const size_t n = (size_t)N * Na;
    double *ds, *pc, *pl = nullptr;
    AIY_TRY(stage_common(c, a, s, P, N, Na, &g->da, &ds, &g->dP));
    AIY_TRY(c->bcast("ege_pc", pc_start, n, C, &pc));
    AIY_TRY(c->room("ge_pk", n * C, &g->pk));
    if (labor) AIY_TRY(c->room("ege_pl", n * C, &pl));
    std::vector<double> dist(C);
    return aiy_egm_solve_batch_dev(c->ws, C, r + sh.c0, w + sh.c0, pc, g->da, ds, g->dP, beta,
                                   sigma, amin, labor, phi, theta, tol, max_iter, g->pk, pl,
                                   iters + sh.c0, dist.data(), status + sh.c0, c->st);
}
}  // namespace

// one device's share of aiy_ge_batch: batched solve, batched chains, outputs back
static int ge_share(GeShare& sh, const double* r, const double* v_rows, const double* a,
                    const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                    double delta, double beta, double sigma, double tol, int64_t max_iter,
                    int64_t z1, double k1, int64_t T, const double* uniforms, double* k_supply,
                    int64_t* iters) {
    AIY_HIP(hipSetDevice(sh.dev));
    GeSolved g;
    double* dU;
    AIY_TRY(ge_stage_uniforms(sh, T, uniforms, &dU));
    AIY_TRY(ge_vfi_solve(sh, r, v_rows, a, s, P, N, Na, alpha, delta, beta, sigma, tol, max_iter,
                         iters, &g));
    std::vector<int> status(sh.cn);
    AIY_TRY(ge_chains(sh, g.pk, g.da, g.dP, dU, N, Na, z1, k1, T, nullptr, k_supply, status.data()));
    return ge_find_empty(sh, status);
}

// one device's share of aiy_egm_ge_batch: the batched EGM solve, the chains of the candidates
// that solved, statuses back
static int egm_ge_share(GeShare& sh, const double* r, const double* w, const double* pc_start,
                        const double* a, const double* s, const double* P, int64_t N, int64_t Na,
                        double beta, double sigma, double amin, int labor, double phi,
                        double theta, double tol, int64_t max_iter, int64_t z1, double k1,
                        int64_t T, const double* uniforms, double* k_supply, int64_t* iters,
                        int32_t* status) {
    AIY_HIP(hipSetDevice(sh.dev));
    GeSolved g;
    double* dU;
    AIY_TRY(ge_stage_uniforms(sh, T, uniforms, &dU));
    AIY_TRY(ge_egm_solve(sh, r, w, pc_start, a, s, P, N, Na, beta, sigma, amin, labor, phi, theta,
                         tol, max_iter, iters, status, &g));
    int32_t* stq = status + sh.c0;
    std::vector<int> empty(sh.cn, 0);
    AIY_TRY(ge_chains(sh, g.pk, g.da, g.dP, dU, N, Na, z1, k1, T, stq, k_supply, empty.data()));
    for (int64_t q = 0; q < sh.cn; ++q) {
        if (!stq[q] && empty[q]) stq[q] = 2;  // find(rand < cumsum(P(z,:))) came up empty
        if (stq[q]) k_supply[sh.c0 + q] = NAN;
    }
    return AIY_OK;
}

// one device's share of aiy_labor_ge_batch: every candidate from the common v_old, incoming
// v_new, policies and index (rows[0..4] [N][Na] doubles, lin0 0-based), the batched labour solve
// at the candidate's own wage, the chains on policy_k
static int labor_ge_share(GeShare& sh, const double* r, const double* const rows[5],
                          const int* lin0, const double* a, const double* s, const double* P,
                          const double* L, int64_t N, int64_t Na, int64_t Nl, double alpha,
                          double delta, double beta, double sigma, double psi, double eta,
                          double tol, int64_t max_iter, int64_t z1, double k1, int64_t T,
                          const double* uniforms, double* k_supply, int64_t* iters) {
    AIY_HIP(hipSetDevice(sh.dev));
    HostCtx* c = sh.ctx;
    const int64_t C = sh.cn;
    const size_t n = (size_t)N * Na;
    double *da, *ds, *dP, *dL, *dU, *d[5];  // d: v_a, v_b, policy_k, policy_l, policy_c
    int* lin;
    AIY_TRY(stage_common(c, a, s, P, N, Na, &da, &ds, &dP));
    AIY_TRY(c->up("L", L, (size_t)Nl, &dL));
    static const char* const names[5] = {"lge_va", "lge_vb", "ge_pk", "lge_pl", "lge_pc"};
    for (int q = 0; q < 5; ++q) AIY_TRY(c->bcast(names[q], rows[q], n, C, &d[q]));
    AIY_TRY(c->bcast("ge_idx", lin0, n, C, &lin));
    AIY_TRY(ge_stage_uniforms(sh, T, uniforms, &dU));
    const std::vector<double> w = ge_wages(sh, r, alpha, delta);
    std::vector<int> which(C);
    AIY_TRY(bell_labor_solve_batch_dev(c->ws, C, r + sh.c0, w.data(), d[0], d[1], da, ds, dP, dL,
                                       beta, sigma, psi, eta, tol, max_iter, 0, lin, d[2], d[3],
                                       d[4], iters + sh.c0, which.data(), c->st));
    std::vector<int> status(C);
    AIY_TRY(ge_chains(sh, d[2], da, dP, dU, N, Na, z1, k1, T, nullptr, k_supply, status.data()));
    return ge_find_empty(sh, status);
}

// The share's batched histogram supply (A10) on its C policies — idx (on-grid, 0-based) or pk
// (lottery) [cn][N][Na] — every candidate with skip[q] == 0 (skip nullable) from the common
// start lam_rows ([N][Na]; NULL: uniform 1/(N·Na)): one batched solve per run of candidates
// that are not skipped; k_supply and dist_iters of [c0, c0 + cn) back (synchronises).
static int ge_hist(GeShare& sh, const GeSolved& g, bool lottery, int64_t N, int64_t Na,
                   double dist_tol, int64_t dist_max_iter, const double* lam_rows,
                   const int32_t* skip, double* k_supply, int64_t* dist_iters) {
    HostCtx* c = sh.ctx;
    const int64_t C = sh.cn;
    const size_t n = (size_t)N * Na;
    double *l0, *l1, *dK;
    std::vector<double> uni;
    if (!lam_rows) {
        uni.assign(n, 1.0 / (double)(N * Na));
        lam_rows = uni.data();
    }
    AIY_TRY(c->bcast("geh_l0", lam_rows, n, C, &l0));
    AIY_TRY(c->room("geh_l1", n * C, &l1));
    AIY_TRY(c->room("geh_K", (size_t)C, &dK));
    for (int64_t q = 0; q < C; ++q)
        if (skip && skip[q]) {
            k_supply[sh.c0 + q] = NAN;
            dist_iters[sh.c0 + q] = 0;
        }
    std::vector<double> dist(C);
    AIY_TRY(ge_runs(C, skip, [&](int64_t q0, int64_t q1) -> int {
        AIY_TRY(aiy_dist_stationary_batch_dev(c->ws, q1 - q0, l0 + q0 * n,
                                              lottery ? nullptr : g.idx + q0 * n,
                                              lottery ? g.pk + q0 * n : nullptr, g.da, g.dP,
                                              dist_tol, dist_max_iter, l1 + q0 * n, dK + q0,
                                              dist_iters + sh.c0 + q0, dist.data() + q0, c->st));
        // a run's K lands at its offset in the caller's array
        return c->down(k_supply + sh.c0 + q0, dK + q0, (size_t)(q1 - q0));
    }));
    return c->sync();  // (uni is the source of an enqueued copy until here)
}

// one device's share of aiy_ge_hist_batch: ge_share with the chains replaced by the batched
// histogram on the solve's index policy
static int ge_hist_share(GeShare& sh, const double* r, const double* v_rows, const double* a,
                         const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                         double delta, double beta, double sigma, double tol, int64_t max_iter,
                         double dist_tol, int64_t dist_max_iter, const double* lam_rows,
                         double* k_supply, int64_t* iters, int64_t* dist_iters) {
    AIY_HIP(hipSetDevice(sh.dev));
    GeSolved g;
    AIY_TRY(ge_vfi_solve(sh, r, v_rows, a, s, P, N, Na, alpha, delta, beta, sigma, tol, max_iter,
                         iters, &g));
    return ge_hist(sh, g, false, N, Na, dist_tol, dist_max_iter, lam_rows, nullptr, k_supply,
                   dist_iters);
}

// one device's share of aiy_egm_ge_hist_batch: egm_ge_share with the chains replaced by the
// batched lottery histogram on policy_k of the candidates that solved
static int egm_ge_hist_share(GeShare& sh, const double* r, const double* w, const double* pc_start,
                             const double* a, const double* s, const double* P, int64_t N,
                             int64_t Na, double beta, double sigma, double amin, int labor,
                             double phi, double theta, double tol, int64_t max_iter,
                             double dist_tol, int64_t dist_max_iter, const double* lam_rows,
                             double* k_supply, int64_t* iters, int64_t* dist_iters,
                             int32_t* status) {
    AIY_HIP(hipSetDevice(sh.dev));
    GeSolved g;
    AIY_TRY(ge_egm_solve(sh, r, w, pc_start, a, s, P, N, Na, beta, sigma, amin, labor, phi, theta,
                         tol, max_iter, iters, status, &g));
    return ge_hist(sh, g, true, N, Na, dist_tol, dist_max_iter, lam_rows, status + sh.c0, k_supply,
                   dist_iters);
}

// an N x Na column-major start as [N][Na] rows; NULL: zeros
static std::vector<double> start_rows(const double* cm, int64_t N, int64_t Na) {
    std::vector<double> rows((size_t)N * Na, 0.0);
    if (cm) cm_to_rows(cm, N, Na, rows.data());
    return rows;
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_ge_batch(const double* r, int64_t C, const double* v_start, const double* a_grid,
                 const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                 double delta, double beta, double sigma, double labor, double tol,
                 int64_t max_iter, int64_t z1, double k1, int64_t T, const double* uniforms,
                 int n_devices, double* k_supply, double* k_demand, int64_t* iters) {
    if (!r || !v_start || !s || !P || !k_supply || !k_demand || !iters || (T > 1 && !uniforms))
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need C >= 1, N >= 1, Na >= 2");
    AIY_TRY(ge_check_chain(T, z1, N, max_iter));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(ge_check_rates(r, C, delta));
    const std::vector<double> rows = start_rows(v_start, N, Na);
    AIY_TRY(ge_run_shares(C, N, Na, 1, n_devices, [&](GeShare& g) {
        return ge_share(g, r, rows.data(), a_grid, s, P, N, Na, alpha, delta, beta, sigma, tol,
                        max_iter, z1, k1, T, uniforms, k_supply, iters);
    }));
    ge_demand(r, C, labor, alpha, delta, k_demand);
    return AIY_OK;
}

int aiy_labor_ge_batch(const double* r, int64_t C, const double* v_start,
                       const double* v_new_start, const double* policy_k_start,
                       const double* policy_l_start, const double* policy_c_start,
                       const int32_t* policy_lin_start, const double* a_grid, const double* s,
                       const double* P, const double* labor_choice, int64_t N, int64_t Na,
                       int64_t Nl, double alpha, double delta, double beta, double sigma,
                       double psi, double eta, double labor, double tol, int64_t max_iter,
                       int64_t z1, double k1, int64_t T, const double* uniforms, int n_devices,
                       double* k_supply, double* k_demand, int64_t* iters) {
    if (!r || !v_start || !s || !P || !labor_choice || !k_supply || !k_demand || !iters ||
        (T > 1 && !uniforms))
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || N < 1 || Na < 2 || Nl < 1)
        return fail(AIY_BAD_SHAPE, "need C >= 1, N >= 1, Na >= 2, Nl >= 1");
    AIY_TRY(ge_check_chain(T, z1, N, max_iter));
    if (!(std::isfinite(psi) && std::isfinite(eta)))
        return fail(AIY_NON_FINITE, "psi and eta must be finite");
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(ge_check_rates(r, C, delta));
    // the common start, N x Na column-major -> [N][Na]; a NULL start is zeros (index: 1)
    const double* const cm[5] = {v_start, v_new_start, policy_k_start, policy_l_start,
                                 policy_c_start};
    std::vector<double> rows[5];
    const double* rp[5];
    for (int q = 0; q < 5; ++q) {
        rows[q] = start_rows(cm[q], N, Na);
        rp[q] = rows[q].data();
    }
    const std::vector<int> lin0 = idx_rows0(policy_lin_start, 1, N, Na);
    AIY_TRY(ge_run_shares(C, N, Na, Nl, n_devices, [&](GeShare& g) {
        return labor_ge_share(g, r, rp, lin0.data(), a_grid, s, P, labor_choice, N, Na, Nl, alpha,
                              delta, beta, sigma, psi, eta, tol, max_iter, z1, k1, T, uniforms,
                              k_supply, iters);
    }));
    ge_demand(r, C, labor, alpha, delta, k_demand);
    return AIY_OK;
}

int aiy_egm_ge_batch(const double* r, const double* w, int64_t C, const double* policy_c_start,
                     const double* a_grid, const double* s, const double* P, int64_t N,
                     int64_t Na, double alpha, double delta, double beta, double sigma,
                     double amin, int labor_flag, double phi, double theta, double labor,
                     double tol, int64_t max_iter, int64_t z1, double k1, int64_t T,
                     const double* uniforms, int n_devices, double* k_supply, double* k_demand,
                     int64_t* iters, int32_t* status) {
    if (!r || !w || !policy_c_start || !s || !P || !k_supply || !k_demand || !iters || !status ||
        (T > 1 && !uniforms))
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need C >= 1, N >= 1, Na >= 2");
    if (N > 16) return fail(AIY_BAD_SHAPE, "EGM kernels support N <= 16 productivity states");
    AIY_TRY(ge_check_chain(T, z1, N, max_iter));
    if (labor_flag && !(std::isfinite(phi) && std::isfinite(theta)))
        return fail(AIY_NON_FINITE, "phi and theta must be finite");
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(ge_check_rates(r, C, delta));
    AIY_TRY(ge_run_shares(C, N, Na, 1, n_devices, [&](GeShare& g) {
        return egm_ge_share(g, r, w, policy_c_start, a_grid, s, P, N, Na, beta, sigma, amin,
                            labor_flag, phi, theta, tol, max_iter, z1, k1, T, uniforms, k_supply,
                            iters, status);
    }));
    ge_demand(r, C, labor, alpha, delta, k_demand);
    return AIY_OK;
}

int aiy_ge_hist_batch(const double* r, int64_t C, const double* v_start, const double* a_grid,
                      const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                      double delta, double beta, double sigma, double labor, double tol,
                      int64_t max_iter, double dist_tol, int64_t dist_max_iter,
                      const double* lambda_start, int n_devices, double* k_supply,
                      double* k_demand, int64_t* iters, int64_t* dist_iters) {
    if (!r || !v_start || !s || !P || !k_supply || !k_demand || !iters || !dist_iters)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need C >= 1, N >= 1, Na >= 2");
    AIY_TRY(ge_check_hist(max_iter, dist_max_iter));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(ge_check_rates(r, C, delta));
    const std::vector<double> rows = start_rows(v_start, N, Na);
    std::vector<double> lrows;
    if (lambda_start) lrows = start_rows(lambda_start, N, Na);
    AIY_TRY(ge_run_shares(C, N, Na, 1, n_devices, [&](GeShare& g) {
        return ge_hist_share(g, r, rows.data(), a_grid, s, P, N, Na, alpha, delta, beta, sigma, tol,
                             max_iter, dist_tol, dist_max_iter,
                             lambda_start ? lrows.data() : nullptr, k_supply, iters, dist_iters);
    }));
    ge_demand(r, C, labor, alpha, delta, k_demand);
    return AIY_OK;
}

int aiy_egm_ge_hist_batch(const double* r, const double* w, int64_t C,
                          const double* policy_c_start, const double* a_grid, const double* s,
                          const double* P, int64_t N, int64_t Na, double alpha, double delta,
                          double beta, double sigma, double amin, int labor_flag, double phi,
                          double theta, double labor, double tol, int64_t max_iter,
                          double dist_tol, int64_t dist_max_iter, const double* lambda_start,
                          int n_devices, double* k_supply, double* k_demand, int64_t* iters,
                          int64_t* dist_iters, int32_t* status) {
    if (!r || !w || !policy_c_start || !s || !P || !k_supply || !k_demand || !iters ||
        !dist_iters || !status)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need C >= 1, N >= 1, Na >= 2");
    if (N > 16) return fail(AIY_BAD_SHAPE, "EGM kernels support N <= 16 productivity states");
    AIY_TRY(ge_check_hist(max_iter, dist_max_iter));
    if (labor_flag && !(std::isfinite(phi) && std::isfinite(theta)))
        return fail(AIY_NON_FINITE, "phi and theta must be finite");
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(ge_check_rates(r, C, delta));
    // lambda_start Na x N column-major == [N][Na]
    AIY_TRY(ge_run_shares(C, N, Na, 1, n_devices, [&](GeShare& g) {
        return egm_ge_hist_share(g, r, w, policy_c_start, a_grid, s, P, N, Na, beta, sigma, amin,
                                 labor_flag, phi, theta, tol, max_iter, dist_tol, dist_max_iter,
                                 lambda_start, k_supply, iters, dist_iters, status);
    }));
    ge_demand(r, C, labor, alpha, delta, k_demand);
    return AIY_OK;
}

}  // extern "C"
