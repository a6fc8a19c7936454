// Transition-path entry points: the backward EGM pass (aiy_egm_backward_batch[_dev]), the forward
// histogram pass (aiy_dist_forward_batch[_dev]) and both on one stream (aiy_transition_batch:
// the period policies stay on the device, the host reads K, status and fail_t).
// Arrays are [N][Na] rows per (path, period) — the EGM scripts' Na x N column-major; P is
// column-major in the host tier (staged as rows), row-major in the device tier.
// The endogenous-labour economy (A5) has the same five entries, aiy_labor_*: the backward pass
// also yields policy_l, the forward pass also H[c][t] = Σ λ_t·(s_j·policy_l_t), the hours in
// efficiency units.
// Everything a host entry can refuse it refuses before it asks for a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "transition.hpp"
#include "ws.hpp"

namespace aiy {

static int check_counts(int64_t C, int64_t T) {
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (T < 1 || T > (1ll << 31) - 2) return fail(AIY_BAD_SHAPE, "T must be in [1, 2^31 - 1)");
    return AIY_OK;
}

// the price paths: r [C][T+1] finite with 1 + r > 0, w [C][T] finite
static int check_prices(int64_t C, int64_t T, const double* r, const double* w) {
    for (int64_t c = 0; c < C; ++c) {
        for (int64_t t = 0; t <= T; ++t) {
            const double x = r[c * (T + 1) + t];
            if (!std::isfinite(x) || !(1 + x > 0))
                return fail(AIY_BAD_ARG, "path %lld, period %lld: r must be finite with 1 + r > 0",
                            (long long)c + 1, (long long)t);
        }
        for (int64_t t = 0; t < T; ++t)
            if (!std::isfinite(w[c * T + t]))
                return fail(AIY_BAD_ARG, "path %lld, period %lld: w must be finite",
                            (long long)c + 1, (long long)t);
    }
    return AIY_OK;
}

static int check_backward_shape(int64_t N, int64_t Na) {
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!egm_backward_fits(N, Na))
        return fail(AIY_BAD_ARG, "backward EGM pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, Na <= 1024, (2N+1)·Na doubles within 160 KiB)");
    return AIY_OK;
}

static int check_forward_shape(int64_t N, int64_t Na) {
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!dist_forward_fits(N, Na))
        return fail(AIY_BAD_ARG, "forward histogram pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.2 KB within 160 KiB)");
    return AIY_OK;
}

static int check_labor_shapes(int64_t N, int64_t Na, bool backward, bool forward) {
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (backward && !labor_egm_backward_fits(N, Na))
        return fail(AIY_BAD_ARG, "backward labour EGM pass: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, Na <= 1024, 3·N·Na doubles within 160 KiB)");
    if (forward && !labor_dist_forward_fits(N, Na))
        return fail(AIY_BAD_ARG, "forward pass with hours: a path's arrays exceed one CU's LDS "
                                 "(N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.3 KB within 160 KiB)");
    return AIY_OK;
}

// the labour first-order condition's parameters: l = (w s u'(c) / phi)^(1/theta)
static int check_labor_params(double phi, double theta) {
    if (!std::isfinite(phi) || !(phi > 0))
        return fail(AIY_BAD_ARG, "phi must be positive and finite");
    if (!std::isfinite(theta) || theta == 0)
        return fail(AIY_BAD_ARG, "theta must be finite and not 0");
    return AIY_OK;
}

// the backward launch; every pointer is the device's
static int backward_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r, const double* w,
                        const double* pcT, bool shared, const double* a, const double* s,
                        const double* P, double beta, double sigma, double amin, double* pk,
                        double* pc, int* status, int* fail_t, hipStream_t st) {
    EgmBackwardArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C; A.T = (int)T;
    A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
    A.beta = beta; A.sigma = sigma; A.amin = amin;
    A.r = r; A.w = w; A.pcT = pcT;
    A.pcT_stride = shared ? 0 : (size_t)ws->N * ws->Na;
    A.a = a; A.s = s; A.P = P; A.pk = pk; A.pc = pc; A.status = status; A.fail_t = fail_t;
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_egm_backward_batch(A, st));
    return ws_timing_end(ws, st);
}

static int labor_backward_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r, const double* w,
                              const double* pcT, bool shared, const double* a, const double* s,
                              const double* P, double beta, double sigma, double phi,
                              double theta, double amin, double* pk, double* pl, double* pc,
                              int* status, int* fail_t, hipStream_t st) {
    EgmBackwardArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C; A.T = (int)T;
    A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
    A.beta = beta; A.sigma = sigma; A.amin = amin; A.phi = phi; A.theta = theta;
    A.r = r; A.w = w; A.pcT = pcT;
    A.pcT_stride = shared ? 0 : (size_t)ws->N * ws->Na;
    A.a = a; A.s = s; A.P = P; A.pk = pk; A.pl = pl; A.pc = pc;
    A.status = status; A.fail_t = fail_t;
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_labor_egm_backward_batch(A, st));
    return ws_timing_end(ws, st);
}

static int labor_forward_dev(aiy_ws* ws, int64_t C, int64_t T, const double* pk, const double* pl,
                             const double* lam0, bool shared, const double* a, const double* s,
                             const double* P, double* K, double* H, double* lamT, int* status,
                             int* fail_t, const int* skip, hipStream_t st) {
    DistForwardArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C; A.T = (int)T;
    A.pk = pk; A.pl = pl; A.lam0 = lam0;
    A.lam0_stride = shared ? 0 : (size_t)ws->N * ws->Na;
    A.a = a; A.s = s; A.P = P; A.K = K; A.H = H; A.lamT = lamT;
    A.status = status; A.fail_t = fail_t; A.skip = skip;
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_labor_dist_forward_batch(A, st));
    return ws_timing_end(ws, st);
}

static int forward_dev(aiy_ws* ws, int64_t C, int64_t T, const double* pk, const double* lam0,
                       bool shared, const double* a, const double* P, double* K, double* lamT,
                       int* status, int* fail_t, const int* skip, hipStream_t st) {
    DistForwardArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C; A.T = (int)T;
    A.pk = pk; A.lam0 = lam0;
    A.lam0_stride = shared ? 0 : (size_t)ws->N * ws->Na;
    A.a = a; A.P = P; A.K = K; A.lamT = lamT; A.status = status; A.fail_t = fail_t; A.skip = skip;
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_dist_forward_batch(A, st));
    return ws_timing_end(ws, st);
}

// status and fail_t of the device tier: the workspace's block back to the caller (synchronises)
static int read_results(aiy_ws* ws, int64_t C, int32_t* status, int32_t* fail_t, hipStream_t st) {
    TransitionBlocks& tb = ws->transition;
    AIY_HIP(hipMemcpyAsync(tb.hres, tb.res, sizeof(int) * 2 * C, hipMemcpyDeviceToHost, st));
    AIY_HIP(hipStreamSynchronize(st));  // the call's one synchronisation
    for (int64_t c = 0; c < C; ++c) {
        status[c] = tb.hres[c];
        fail_t[c] = tb.hres[C + c];
    }
    return AIY_OK;
}

// what the three host entries stage alike
struct TransitionStaged {
    double *a, *s, *P;
    int* res;  // device [2][C]: status, fail_t
};
static int stage_transition(HostCtx* c, int64_t C, const double* a_grid, const double* s,
                            const double* P, int64_t N, int64_t Na, TransitionStaged* D) {
    std::vector<double> s1(N, 1.0);  // (the forward pass reads a and P only)
    AIY_TRY(stage_common(c, a_grid, s ? s : s1.data(), P, N, Na, &D->a, &D->s, &D->P));
    return c->room("tr_res", 2 * (size_t)C, &D->res);
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_egm_backward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r, const double* w,
                               const double* pc_T, int pc_T_shared, const double* a_grid,
                               const double* s, const double* P, double beta, double sigma,
                               double amin, double* policy_k, double* policy_c, int32_t* status,
                               int32_t* fail_t, void* stream) {
    if (!ws || !r || !w || !pc_T || !a_grid || !s || !P || !policy_k || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_backward_shape(ws->N, ws->Na));
    AIY_TRY(check_prices(C, T, r, w));
    hipStream_t st = (hipStream_t)stream;
    TransitionBlocks& tb = ws->transition;
    AIY_TRY(tb.ensure((size_t)C, (size_t)T));
    const size_t nr = (size_t)C * (T + 1), nw = (size_t)C * T;
    std::memcpy(tb.hrw.get(), r, sizeof(double) * nr);
    std::memcpy(tb.hrw.get() + nr, w, sizeof(double) * nw);
    AIY_HIP(hipMemcpyAsync(tb.rw, tb.hrw, sizeof(double) * (nr + nw), hipMemcpyHostToDevice, st));
    AIY_TRY(backward_dev(ws, C, T, tb.rw, tb.rw + nr, pc_T, pc_T_shared != 0, a_grid, s, P, beta,
                         sigma, amin, policy_k, policy_c, tb.res, tb.res + C, st));
    return read_results(ws, C, status, fail_t, st);
}

int aiy_dist_forward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                               const double* lambda0, int lambda0_shared, const double* a_grid,
                               const double* P, double* K, double* lambda_T, int32_t* status,
                               int32_t* fail_t, void* stream) {
    if (!ws || !policy_k || !lambda0 || !a_grid || !P || !K || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_forward_shape(ws->N, ws->Na));
    hipStream_t st = (hipStream_t)stream;
    TransitionBlocks& tb = ws->transition;
    AIY_TRY(tb.ensure((size_t)C, (size_t)T));
    AIY_TRY(forward_dev(ws, C, T, policy_k, lambda0, lambda0_shared != 0, a_grid, P, K, lambda_T,
                        tb.res, tb.res + C, nullptr, st));
    return read_results(ws, C, status, fail_t, st);
}

int aiy_egm_backward_batch(int64_t C, int64_t T, const double* r, const double* w,
                           const double* pc_T, int pc_T_shared, const double* a_grid,
                           const double* s, const double* P, int64_t N, int64_t Na, double beta,
                           double sigma, double amin, double* policy_k, double* policy_c,
                           int32_t* status, int32_t* fail_t) {
    if (!r || !w || !pc_T || !s || !P || !policy_k || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_backward_shape(N, Na));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(check_prices(C, T, r, w));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, s, P, N, Na, &D));
    const size_t n = (size_t)N * Na, np = (size_t)C * T * n;
    double *dr, *dw, *dc, *dpk, *dpc = nullptr;
    AIY_TRY(c->up("tr_r", r, (size_t)C * (T + 1), &dr));
    AIY_TRY(c->up("tr_w", w, (size_t)C * T, &dw));
    AIY_TRY(c->up("tr_pcT", pc_T, pc_T_shared ? n : n * (size_t)C, &dc));
    AIY_TRY(c->room("tr_pk", np, &dpk));
    if (policy_c) AIY_TRY(c->room("tr_pc", np, &dpc));
    AIY_TRY(backward_dev(c->ws, C, T, dr, dw, dc, pc_T_shared != 0, D.a, D.s, D.P, beta, sigma,
                         amin, dpk, dpc, D.res, D.res + C, c->st));
    AIY_TRY(c->down(policy_k, dpk, np));
    if (policy_c) AIY_TRY(c->down(policy_c, dpc, np));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

int aiy_dist_forward_batch(int64_t C, int64_t T, const double* policy_k, const double* lambda0,
                           int lambda0_shared, const double* a_grid, const double* P, int64_t N,
                           int64_t Na, double* K, double* lambda_T, int32_t* status,
                           int32_t* fail_t) {
    if (!policy_k || !lambda0 || !P || !K || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_forward_shape(N, Na));
    AIY_TRY(check_grid_strict(a_grid, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, nullptr, P, N, Na, &D));
    const size_t n = (size_t)N * Na;
    double *dpk, *dl0, *dK, *dlT = nullptr;
    AIY_TRY(c->up("tr_pk", policy_k, (size_t)C * T * n, &dpk));
    AIY_TRY(c->up("tr_l0", lambda0, lambda0_shared ? n : n * (size_t)C, &dl0));
    AIY_TRY(c->room("tr_K", (size_t)C * (T + 1), &dK));
    if (lambda_T) AIY_TRY(c->room("tr_lT", n * (size_t)C, &dlT));
    AIY_TRY(forward_dev(c->ws, C, T, dpk, dl0, lambda0_shared != 0, D.a, D.P, dK, dlT, D.res,
                        D.res + C, nullptr, c->st));
    AIY_TRY(c->down(K, dK, (size_t)C * (T + 1)));
    if (lambda_T) AIY_TRY(c->down(lambda_T, dlT, n * (size_t)C));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

int aiy_transition_batch(int64_t C, int64_t T, const double* r, const double* w,
                         const double* pc_T, int pc_T_shared, const double* lambda0,
                         int lambda0_shared, const double* a_grid, const double* s,
                         const double* P, int64_t N, int64_t Na, double beta, double sigma,
                         double amin, double* K, int32_t* status, int32_t* fail_t) {
    if (!r || !w || !pc_T || !lambda0 || !s || !P || !K || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_backward_shape(N, Na));
    AIY_TRY(check_forward_shape(N, Na));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(check_prices(C, T, r, w));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, s, P, N, Na, &D));
    const size_t n = (size_t)N * Na;
    double *dr, *dw, *dc, *dl0, *dpk, *dK;
    AIY_TRY(c->up("tr_r", r, (size_t)C * (T + 1), &dr));
    AIY_TRY(c->up("tr_w", w, (size_t)C * T, &dw));
    AIY_TRY(c->up("tr_pcT", pc_T, pc_T_shared ? n : n * (size_t)C, &dc));
    AIY_TRY(c->up("tr_l0", lambda0, lambda0_shared ? n : n * (size_t)C, &dl0));
    AIY_TRY(c->room("tr_pk", (size_t)C * T * n, &dpk));
    AIY_TRY(c->room("tr_K", (size_t)C * (T + 1), &dK));
    AIY_TRY(backward_dev(c->ws, C, T, dr, dw, dc, pc_T_shared != 0, D.a, D.s, D.P, beta, sigma,
                         amin, dpk, nullptr, D.res, D.res + C, c->st));
    // a path the backward pass stopped keeps its status and fail_t; its K is NaN
    AIY_TRY(forward_dev(c->ws, C, T, dpk, dl0, lambda0_shared != 0, D.a, D.P, dK, nullptr, D.res,
                        D.res + C, D.res, c->st));
    AIY_TRY(c->down(K, dK, (size_t)C * (T + 1)));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

int aiy_labor_egm_backward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r,
                                     const double* w, const double* pc_T, int pc_T_shared,
                                     const double* a_grid, const double* s, const double* P,
                                     double beta, double sigma, double phi, double theta,
                                     double amin, double* policy_k, double* policy_l,
                                     double* policy_c, int32_t* status, int32_t* fail_t,
                                     void* stream) {
    if (!ws || !r || !w || !pc_T || !a_grid || !s || !P || !policy_k || !policy_l || !status ||
        !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_labor_shapes(ws->N, ws->Na, true, false));
    AIY_TRY(check_labor_params(phi, theta));
    AIY_TRY(check_prices(C, T, r, w));
    hipStream_t st = (hipStream_t)stream;
    TransitionBlocks& tb = ws->transition;
    AIY_TRY(tb.ensure((size_t)C, (size_t)T));
    const size_t nr = (size_t)C * (T + 1), nw = (size_t)C * T;
    std::memcpy(tb.hrw.get(), r, sizeof(double) * nr);
    std::memcpy(tb.hrw.get() + nr, w, sizeof(double) * nw);
    AIY_HIP(hipMemcpyAsync(tb.rw, tb.hrw, sizeof(double) * (nr + nw), hipMemcpyHostToDevice, st));
    AIY_TRY(labor_backward_dev(ws, C, T, tb.rw, tb.rw + nr, pc_T, pc_T_shared != 0, a_grid, s, P,
                               beta, sigma, phi, theta, amin, policy_k, policy_l, policy_c, tb.res,
                               tb.res + C, st));
    return read_results(ws, C, status, fail_t, st);
}

int aiy_labor_dist_forward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                                     const double* policy_l, const double* lambda0,
                                     int lambda0_shared, const double* a_grid, const double* s,
                                     const double* P, double* K, double* H, double* lambda_T,
                                     int32_t* status, int32_t* fail_t, void* stream) {
    if (!ws || !policy_k || !policy_l || !lambda0 || !a_grid || !s || !P || !K || !H || !status ||
        !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_labor_shapes(ws->N, ws->Na, false, true));
    hipStream_t st = (hipStream_t)stream;
    TransitionBlocks& tb = ws->transition;
    AIY_TRY(tb.ensure((size_t)C, (size_t)T));
    AIY_TRY(labor_forward_dev(ws, C, T, policy_k, policy_l, lambda0, lambda0_shared != 0, a_grid,
                              s, P, K, H, lambda_T, tb.res, tb.res + C, nullptr, st));
    return read_results(ws, C, status, fail_t, st);
}

int aiy_labor_egm_backward_batch(int64_t C, int64_t T, const double* r, const double* w,
                                 const double* pc_T, int pc_T_shared, const double* a_grid,
                                 const double* s, const double* P, int64_t N, int64_t Na,
                                 double beta, double sigma, double phi, double theta, double amin,
                                 double* policy_k, double* policy_l, double* policy_c,
                                 int32_t* status, int32_t* fail_t) {
    if (!r || !w || !pc_T || !s || !P || !policy_k || !policy_l || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_labor_shapes(N, Na, true, false));
    AIY_TRY(check_labor_params(phi, theta));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(check_prices(C, T, r, w));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, s, P, N, Na, &D));
    const size_t n = (size_t)N * Na, np = (size_t)C * T * n;
    double *dr, *dw, *dc, *dpk, *dpl, *dpc = nullptr;
    AIY_TRY(c->up("tr_r", r, (size_t)C * (T + 1), &dr));
    AIY_TRY(c->up("tr_w", w, (size_t)C * T, &dw));
    AIY_TRY(c->up("tr_pcT", pc_T, pc_T_shared ? n : n * (size_t)C, &dc));
    AIY_TRY(c->room("tr_pk", np, &dpk));
    AIY_TRY(c->room("tr_pl", np, &dpl));
    if (policy_c) AIY_TRY(c->room("tr_pc", np, &dpc));
    AIY_TRY(labor_backward_dev(c->ws, C, T, dr, dw, dc, pc_T_shared != 0, D.a, D.s, D.P, beta,
                               sigma, phi, theta, amin, dpk, dpl, dpc, D.res, D.res + C, c->st));
    AIY_TRY(c->down(policy_k, dpk, np));
    AIY_TRY(c->down(policy_l, dpl, np));
    if (policy_c) AIY_TRY(c->down(policy_c, dpc, np));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

int aiy_labor_dist_forward_batch(int64_t C, int64_t T, const double* policy_k,
                                 const double* policy_l, const double* lambda0,
                                 int lambda0_shared, const double* a_grid, const double* s,
                                 const double* P, int64_t N, int64_t Na, double* K, double* H,
                                 double* lambda_T, int32_t* status, int32_t* fail_t) {
    if (!policy_k || !policy_l || !lambda0 || !s || !P || !K || !H || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_labor_shapes(N, Na, false, true));
    AIY_TRY(check_grid_strict(a_grid, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, s, P, N, Na, &D));
    const size_t n = (size_t)N * Na;
    double *dpk, *dpl, *dl0, *dK, *dH, *dlT = nullptr;
    AIY_TRY(c->up("tr_pk", policy_k, (size_t)C * T * n, &dpk));
    AIY_TRY(c->up("tr_pl", policy_l, (size_t)C * T * n, &dpl));
    AIY_TRY(c->up("tr_l0", lambda0, lambda0_shared ? n : n * (size_t)C, &dl0));
    AIY_TRY(c->room("tr_K", (size_t)C * (T + 1), &dK));
    AIY_TRY(c->room("tr_H", (size_t)C * T, &dH));
    if (lambda_T) AIY_TRY(c->room("tr_lT", n * (size_t)C, &dlT));
    AIY_TRY(labor_forward_dev(c->ws, C, T, dpk, dpl, dl0, lambda0_shared != 0, D.a, D.s, D.P, dK,
                              dH, dlT, D.res, D.res + C, nullptr, c->st));
    AIY_TRY(c->down(K, dK, (size_t)C * (T + 1)));
    AIY_TRY(c->down(H, dH, (size_t)C * T));
    if (lambda_T) AIY_TRY(c->down(lambda_T, dlT, n * (size_t)C));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

int aiy_labor_transition_batch(int64_t C, int64_t T, const double* r, const double* w,
                               const double* pc_T, int pc_T_shared, const double* lambda0,
                               int lambda0_shared, const double* a_grid, const double* s,
                               const double* P, int64_t N, int64_t Na, double beta, double sigma,
                               double phi, double theta, double amin, double* K, double* H,
                               int32_t* status, int32_t* fail_t) {
    if (!r || !w || !pc_T || !lambda0 || !s || !P || !K || !H || !status || !fail_t)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_counts(C, T));
    AIY_TRY(check_labor_shapes(N, Na, true, true));
    AIY_TRY(check_labor_params(phi, theta));
    AIY_TRY(check_grid_strict(a_grid, Na));
    AIY_TRY(check_prices(C, T, r, w));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    TransitionStaged D;
    AIY_TRY(stage_transition(c, C, a_grid, s, P, N, Na, &D));
    const size_t n = (size_t)N * Na;
    double *dr, *dw, *dc, *dl0, *dpk, *dpl, *dK, *dH;
    AIY_TRY(c->up("tr_r", r, (size_t)C * (T + 1), &dr));
    AIY_TRY(c->up("tr_w", w, (size_t)C * T, &dw));
    AIY_TRY(c->up("tr_pcT", pc_T, pc_T_shared ? n : n * (size_t)C, &dc));
    AIY_TRY(c->up("tr_l0", lambda0, lambda0_shared ? n : n * (size_t)C, &dl0));
    AIY_TRY(c->room("tr_pk", (size_t)C * T * n, &dpk));
    AIY_TRY(c->room("tr_pl", (size_t)C * T * n, &dpl));
    AIY_TRY(c->room("tr_K", (size_t)C * (T + 1), &dK));
    AIY_TRY(c->room("tr_H", (size_t)C * T, &dH));
    AIY_TRY(labor_backward_dev(c->ws, C, T, dr, dw, dc, pc_T_shared != 0, D.a, D.s, D.P, beta,
                               sigma, phi, theta, amin, dpk, dpl, nullptr, D.res, D.res + C,
                               c->st));
    // a path the backward pass stopped keeps its status and fail_t; its K and H are NaN
    AIY_TRY(labor_forward_dev(c->ws, C, T, dpk, dpl, dl0, lambda0_shared != 0, D.a, D.s, D.P, dK,
                              dH, nullptr, D.res, D.res + C, D.res, c->st));
    AIY_TRY(c->down(K, dK, (size_t)C * (T + 1)));
    AIY_TRY(c->down(H, dH, (size_t)C * T));
    AIY_TRY(c->down(status, D.res, (size_t)C));
    AIY_TRY(c->down(fail_t, D.res + C, (size_t)C));
    return c->sync();
}

}  // extern "C"
