// Sequence-space Jacobian entry points: the expectation vectors (aiy_dist_expect_batch[_dev]), the
// fake-news contraction (aiy_ssj_fake_news[_dev]) and the whole Jacobian of the capital path in
// r and w on one stream (aiy_ssj_jacobian: the period policies, Λ1, E and F stay on the device),
// the same of C economies, each stage one launch over a chunk of them (aiy_ssj_jacobian_batch),
// and the same of the labour economy's capital and hours paths (aiy_ssj_jacobian_labor).
// Arrays are [N][Na] rows per block; P is column-major in the host tier (staged as rows),
// row-major in the device tier.  Everything a host entry can refuse it refuses before it asks
// for a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "ssj.hpp"
#include "transition.hpp"
#include "ws.hpp"

namespace aiy {

static int check_expect_counts(int64_t C, int64_t T) {
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (T < 1 || T > (1ll << 31) - 2) return fail(AIY_BAD_SHAPE, "T must be in [1, 2^31 - 1)");
    return AIY_OK;
}

static int check_expect_shape(int64_t N, int64_t Na) {
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!dist_expect_fits(N, Na))
        return fail(AIY_BAD_ARG, "expectation pass: a steady state's arrays exceed one CU's LDS "
                                 "(N <= 16, 28·N·Na + 2 KB within 160 KiB)");
    return AIY_OK;
}

static int check_fake_news(int64_t T, int64_t n_in, int64_t n, double h) {
    if (T < 1 || T > kSsjMaxT) return fail(AIY_BAD_SHAPE, "T must be in [1, 32768]");
    if (n_in < 1 || n_in > 65535) return fail(AIY_BAD_SHAPE, "need 1 <= n_in <= 65535");
    if (n < 1 || n > (1ll << 28)) return fail(AIY_BAD_SHAPE, "need 1 <= n <= 2^28");
    if (!(h > 0) || !std::isfinite(h)) return fail(AIY_BAD_ARG, "h must be positive and finite");
    return AIY_OK;
}

static int expect_dev(int64_t N, int64_t Na, int64_t C, int64_t T, const double* pk,
                      const double* y0, bool shared, const double* a, const double* P, double* E,
                      hipStream_t st) {
    DistExpectArgs A{};
    A.N = (int)N; A.Na = (int)Na; A.C = (int)C; A.T = (int)T;
    A.pk = pk; A.y0 = y0;
    A.y0_stride = shared ? 0 : (size_t)N * Na;
    A.a = a; A.P = P; A.E = E;
    return launch_dist_expect_batch(A, st);
}

static int fake_news_dev(int64_t T, int64_t n_in, int64_t n, const double* E, const double* lam1,
                         double h, double* F, double* J, hipStream_t st) {
    SsjFakeNewsArgs A{};
    A.T = (int)T; A.n_in = (int)n_in; A.n = (int)n; A.h = h;
    A.E = E; A.lam1 = lam1; A.F = F; A.J = J;
    return launch_ssj_fake_news(A, st);
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_dist_expect_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                              const double* y0, int y0_shared, const double* a_grid,
                              const double* P, double* E, void* stream) {
    if (!ws || !policy_k || !y0 || !a_grid || !P || !E) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_expect_counts(C, T));
    AIY_TRY(check_expect_shape(ws->N, ws->Na));
    return expect_dev(ws->N, ws->Na, C, T, policy_k, y0, y0_shared != 0, a_grid, P, E,
                      (hipStream_t)stream);
}

int aiy_dist_expect_batch(int64_t C, int64_t T, const double* policy_k, const double* y0,
                          int y0_shared, const double* a_grid, const double* P, int64_t N,
                          int64_t Na, double* E) {
    if (!policy_k || !y0 || !P || !E) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_expect_counts(C, T));
    AIY_TRY(check_expect_shape(N, Na));
    AIY_TRY(check_grid_strict(a_grid, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    std::vector<double> s1(N, 1.0);  // (the pass reads a and P only)
    double *da, *ds, *dP, *dpk, *dy, *dE;
    AIY_TRY(stage_common(c, a_grid, s1.data(), P, N, Na, &da, &ds, &dP));
    const size_t n = (size_t)N * Na;
    AIY_TRY(c->up("ssj_pk", policy_k, n * (size_t)C, &dpk));
    AIY_TRY(c->up("ssj_y0", y0, y0_shared ? n : n * (size_t)C, &dy));
    AIY_TRY(c->room("ssj_E", n * (size_t)C * T, &dE));
    AIY_TRY(expect_dev(N, Na, C, T, dpk, dy, y0_shared != 0, da, dP, dE, c->st));
    AIY_TRY(c->down(E, dE, n * (size_t)C * T));
    return c->sync();
}

int aiy_ssj_fake_news_dev(int64_t T, int64_t n_in, int64_t n, const double* E, const double* lam1,
                          double h, double* F, double* J, void* stream) {
    if (!E || !lam1 || !F || !J) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_fake_news(T, n_in, n, h));
    return fake_news_dev(T, n_in, n, E, lam1, h, F, J, (hipStream_t)stream);
}

int aiy_ssj_fake_news(int64_t T, int64_t n_in, int64_t n, const double* E, const double* lam1,
                      double h, double* F, double* J) {
    if (!E || !lam1 || !F || !J) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_fake_news(T, n_in, n, h));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(1, n < 2 ? 2 : n, 1, &c));
    const size_t tn = (size_t)T * n, tt = (size_t)T * T * n_in;
    double *dE, *dl, *dF, *dJ;
    AIY_TRY(c->up("ssj_E", E, tn, &dE));
    AIY_TRY(c->up("ssj_lam1", lam1, tn * (size_t)(n_in + 1), &dl));
    AIY_TRY(c->room("ssj_F", tt, &dF));
    AIY_TRY(c->room("ssj_J", tt, &dJ));
    AIY_TRY(fake_news_dev(T, n_in, n, dE, dl, h, dF, dJ, c->st));
    AIY_TRY(c->down(F, dF, tt));
    AIY_TRY(c->down(J, dJ, tt));
    return c->sync();
}

int aiy_ssj_jacobian(const double* policy_c, const double* lambda, double r_ss, double w_ss,
                     const double* a_grid, const double* s, const double* P, int64_t N,
                     int64_t Na, double beta, double sigma, double amin, int64_t T, double h,
                     double* J_r, double* J_w, double* F_r, double* F_w, double* E,
                     int32_t* backward_status, int32_t* forward_status, double* stage_ms) {
    if (!policy_c || !lambda || !s || !P || !J_r || !J_w || !backward_status || !forward_status)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!egm_backward_fits(N, Na) || !dist_forward_fits(N, Na))
        return fail(AIY_BAD_ARG, "Jacobian: the transition passes' arrays exceed one CU's LDS "
                                 "(aiy_transition_batch's fit rules)");
    AIY_TRY(check_expect_shape(N, Na));
    AIY_TRY(check_fake_news(T, 2, N * Na, h));
    AIY_TRY(check_grid_strict(a_grid, Na));
    if (!std::isfinite(r_ss) || !(1 + r_ss > 0) || !std::isfinite(r_ss + h))
        return fail(AIY_BAD_ARG, "r_ss must be finite with 1 + r_ss > 0");
    if (!std::isfinite(w_ss) || !std::isfinite(w_ss + h))
        return fail(AIY_BAD_ARG, "w_ss must be finite");
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    double *da, *ds, *dP;
    AIY_TRY(stage_common(c, a_grid, s, P, N, Na, &da, &ds, &dP));
    const size_t n = (size_t)N * Na, tt = (size_t)T * T;
    const int64_t C3 = 3, CF = 3 * T;
    // the three price paths: the steady state, r[T-1] + h, w[T-1] + h
    std::vector<double> rp(C3 * (T + 1), r_ss), wp(C3 * T, w_ss), y0(n);
    rp[(size_t)(T + 1) + T - 1] = r_ss + h;
    wp[2 * (size_t)T + T - 1] = w_ss + h;
    for (size_t e = 0; e < n; ++e) y0[e] = a_grid[e % Na];
    double *dr, *dw, *dc, *dl0, *dy, *dpk, *dK, *dl1, *dE, *dF, *dJ;
    int *bres, *fres;
    AIY_TRY(c->up_own("tr_r", std::move(rp), &dr));
    AIY_TRY(c->up_own("tr_w", std::move(wp), &dw));
    AIY_TRY(c->up_own("ssj_y0", std::move(y0), &dy));
    AIY_TRY(c->up("tr_pcT", policy_c, n, &dc));
    AIY_TRY(c->up("tr_l0", lambda, n, &dl0));
    AIY_TRY(c->room("tr_pk", (size_t)C3 * T * n, &dpk));
    AIY_TRY(c->room("tr_K", (size_t)CF * 2, &dK));
    AIY_TRY(c->room("ssj_lam1", (size_t)CF * n, &dl1));
    AIY_TRY(c->room("ssj_E", (size_t)T * n, &dE));
    AIY_TRY(c->room("ssj_F", 2 * tt, &dF));
    AIY_TRY(c->room("ssj_J", 2 * tt, &dJ));
    AIY_TRY(c->room("ssj_bres", 2 * (size_t)C3, &bres));
    AIY_TRY(c->room("ssj_fres", 2 * (size_t)CF, &fres));
    Events ev;  // the stages' boundaries as the stream dispatches them
    if (stage_ms) AIY_TRY(ev.create(5, 0));
    auto mark = [&](int q) -> int {
        if (stage_ms) AIY_HIP(hipEventRecord(ev[q], c->st));
        return AIY_OK;
    };
    AIY_TRY(mark(0));
    {  // 1. the policies of an agent who learns of the change s periods ahead: pk [3][T][N][Na]
        EgmBackwardArgs A{};
        A.N = (int)N; A.Na = (int)Na; A.C = (int)C3; A.T = (int)T;
        A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
        A.beta = beta; A.sigma = sigma; A.amin = amin;
        A.r = dr; A.w = dw; A.pcT = dc; A.pcT_stride = 0;
        A.a = da; A.s = ds; A.P = dP; A.pk = dpk; A.pc = nullptr;
        A.status = bres; A.fail_t = bres + C3;
        AIY_TRY(launch_egm_backward_batch(A, c->st));
    }
    AIY_TRY(mark(1));
    {  // 2. one push of the steady state's λ through each of them: Λ1 [3][T][N][Na]
        DistForwardArgs A{};
        A.N = (int)N; A.Na = (int)Na; A.C = (int)CF; A.T = 1;
        A.pk = dpk; A.lam0 = dl0; A.lam0_stride = 0;
        A.a = da; A.P = dP; A.K = dK; A.lamT = dl1;
        A.status = fres; A.fail_t = fres + CF; A.skip = nullptr;
        AIY_TRY(launch_dist_forward_batch(A, c->st));
    }
    AIY_TRY(mark(2));
    // 3. the expectation vectors of the base path's period-0 policy
    AIY_TRY(expect_dev(N, Na, 1, T, dpk, dy, true, da, dP, dE, c->st));
    AIY_TRY(mark(3));
    // 4, 5. the fake-news matrices and the Jacobians
    AIY_TRY(fake_news_dev(T, 2, (int64_t)n, dE, dl1, h, dF, dJ, c->st));
    AIY_TRY(mark(4));
    std::vector<int> hb(C3), hf(CF);
    AIY_TRY(c->down(J_r, dJ, tt));
    AIY_TRY(c->down(J_w, dJ + tt, tt));
    if (F_r) AIY_TRY(c->down(F_r, dF, tt));
    if (F_w) AIY_TRY(c->down(F_w, dF + tt, tt));
    if (E) AIY_TRY(c->down(E, dE, (size_t)T * n));
    AIY_TRY(c->down(hb.data(), bres, (size_t)C3));
    AIY_TRY(c->down(hf.data(), fres, (size_t)CF));
    AIY_TRY(c->sync());
    int sb = 0, sf = 0;
    for (int v : hb) sb |= v;
    for (int v : hf) sf |= v;
    *backward_status = sb;
    *forward_status = sf;
    if (sb | sf) {  // a pass stopped: nothing downstream of it is a derivative
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t q = 0; q < tt; ++q) J_r[q] = J_w[q] = nan;
    }
    if (stage_ms)
        for (int q = 0; q < 4; ++q) {
            float ms = 0;
            AIY_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            stage_ms[q] = ms;
        }
    return AIY_OK;
}

int aiy_ssj_jacobian_batch(int64_t C, const double* policy_c, const double* lambda,
                           const double* r_ss, const double* w_ss, const double* a_grid,
                           const double* s, const double* P, int64_t N, int64_t Na,
                           const double* beta, const double* sigma, const double* amin, int64_t T,
                           double h, double* J_r, double* J_w, double* F_r, double* F_w, double* E,
                           int32_t* backward_status, int32_t* forward_status, double* stage_ms,
                           int64_t chunk) {
    if (!policy_c || !lambda || !r_ss || !w_ss || !a_grid || !s || !P || !beta || !sigma ||
        !amin || !J_r || !J_w || !backward_status || !forward_status)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || C > (1ll << 24)) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 2^24");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!egm_backward_fits(N, Na) || !dist_forward_fits(N, Na))
        return fail(AIY_BAD_ARG, "Jacobian: the transition passes' arrays exceed one CU's LDS "
                                 "(aiy_transition_batch's fit rules)");
    AIY_TRY(check_expect_shape(N, Na));
    AIY_TRY(check_fake_news(T, 2, N * Na, h));
    if (chunk < 0 || chunk > kSsjBatchMaxChunk)
        return fail(AIY_BAD_ARG, "chunk must be in [0, 32767] (0: the default)");
    for (int64_t e = 0; e < C; ++e) {
        const long long q = (long long)e;
        if (const int rc = check_grid_strict(a_grid + e * Na, Na)) {
            const std::string why = aiy_last_error();
            return fail(rc, "economy %lld: %s", q, why.c_str());
        }
        if (!std::isfinite(r_ss[e]) || !(1 + r_ss[e] > 0) || !std::isfinite(r_ss[e] + h))
            return fail(AIY_BAD_ARG, "economy %lld: r_ss must be finite with 1 + r_ss > 0", q);
        if (!std::isfinite(w_ss[e]) || !std::isfinite(w_ss[e] + h))
            return fail(AIY_BAD_ARG, "economy %lld: w_ss must be finite", q);
        if (!std::isfinite(beta[e]) || !(beta[e] > 0))
            return fail(AIY_BAD_ARG, "economy %lld: beta must be positive and finite", q);
        if (!std::isfinite(sigma[e]) || !(sigma[e] > 0))
            return fail(AIY_BAD_ARG, "economy %lld: sigma must be positive and finite", q);
        if (!std::isfinite(amin[e])) return fail(AIY_BAD_ARG, "economy %lld: amin must be finite", q);
    }
    const size_t n = (size_t)N * Na, tt = (size_t)T * T, NN = (size_t)N * N;
    if (chunk == 0) {  // pk and Λ1 (3·T·n each), E (T·n), F and J (2·T² each) of an economy
        const size_t per = sizeof(double) * (7 * (size_t)T * n + 4 * tt);
        chunk = (int64_t)std::max<size_t>(1, kBatchStageBytes / per);
    }
    chunk = std::min(std::min(chunk, C), kSsjBatchMaxChunk);
    chunk = std::min(chunk, std::max<int64_t>(1, ((1ll << 31) - 1) / (3 * T)));  // 3·T paths each
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    Events ev;  // the stages' boundaries as the stream dispatches them, chunk by chunk
    if (stage_ms) {
        AIY_TRY(ev.create(5, 0));
        for (int q = 0; q < 4; ++q) stage_ms[q] = 0;
    }
    auto mark = [&](int q) -> int {
        if (stage_ms) AIY_HIP(hipEventRecord(ev[q], c->st));
        return AIY_OK;
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t e0 = 0; e0 < C; e0 += chunk) {
        const int64_t m = std::min(chunk, C - e0), C3 = 3 * m, CF = 3 * m * T;
        // an economy's three price paths: the steady state, r[T-1] + h, w[T-1] + h
        std::vector<double> rp(C3 * (T + 1)), wp(C3 * T), y0(m * n), prm(3 * m);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t e = e0 + i;
            std::fill_n(rp.begin() + 3 * i * (T + 1), 3 * (T + 1), r_ss[e]);
            std::fill_n(wp.begin() + 3 * i * T, 3 * T, w_ss[e]);
            rp[(size_t)(3 * i + 1) * (T + 1) + T - 1] = r_ss[e] + h;
            wp[(size_t)(3 * i + 2) * T + T - 1] = w_ss[e] + h;
            for (size_t k = 0; k < n; ++k) y0[i * n + k] = a_grid[e * Na + k % Na];
            prm[3 * i] = beta[e];
            prm[3 * i + 1] = sigma[e];
            prm[3 * i + 2] = amin[e];
        }
        double *da, *ds, *dP, *dprm, *dr, *dw, *dc, *dl0, *dy, *dpk, *dK, *dl1, *dE, *dF, *dJ;
        int *bres, *fres;
        AIY_TRY(c->up("ssjb_a", a_grid + e0 * Na, (size_t)m * Na, &da));
        AIY_TRY(c->up("ssjb_s", s + e0 * N, (size_t)m * N, &ds));
        AIY_TRY(c->up_rows("ssjb_P", P + e0 * NN, N, N, m, &dP));
        AIY_TRY(c->up_own("ssjb_prm", std::move(prm), &dprm));
        AIY_TRY(c->up_own("tr_r", std::move(rp), &dr));
        AIY_TRY(c->up_own("tr_w", std::move(wp), &dw));
        AIY_TRY(c->up_own("ssj_y0", std::move(y0), &dy));
        AIY_TRY(c->up("tr_pcT", policy_c + e0 * n, (size_t)m * n, &dc));
        AIY_TRY(c->up("tr_l0", lambda + e0 * n, (size_t)m * n, &dl0));
        AIY_TRY(c->room("tr_pk", (size_t)C3 * T * n, &dpk));
        AIY_TRY(c->room("tr_K", (size_t)CF * 2, &dK));
        AIY_TRY(c->room("ssj_lam1", (size_t)CF * n, &dl1));
        AIY_TRY(c->room("ssj_E", (size_t)m * T * n, &dE));
        AIY_TRY(c->room("ssj_F", 2 * tt * m, &dF));
        AIY_TRY(c->room("ssj_J", 2 * tt * m, &dJ));
        AIY_TRY(c->room("ssj_bres", 2 * (size_t)C3, &bres));
        AIY_TRY(c->room("ssj_fres", 2 * (size_t)CF, &fres));
        AIY_TRY(mark(0));
        {  // 1. pk [m][3][T][N][Na], path 3i + p with economy i's parameters, grid and shocks
            EgmBackwardArgs A{};
            A.N = (int)N; A.Na = (int)Na; A.C = (int)C3; A.T = (int)T;
            A.group = 3; A.prm = dprm;
            A.a_stride = (size_t)Na; A.s_stride = (size_t)N; A.P_stride = NN;
            A.r = dr; A.w = dw; A.pcT = dc; A.pcT_stride = 0; A.pcT_estride = n;
            A.a = da; A.s = ds; A.P = dP; A.pk = dpk; A.pc = nullptr;
            A.status = bres; A.fail_t = bres + C3;
            AIY_TRY(launch_egm_backward_batch(A, c->st));
        }
        AIY_TRY(mark(1));
        {  // 2. Λ1 [m][3][T][N][Na]: one push of economy i's λ through each of its 3T policies
            DistForwardArgs A{};
            A.N = (int)N; A.Na = (int)Na; A.C = (int)CF; A.T = 1;
            A.group = (int)(3 * T); A.a_stride = (size_t)Na; A.P_stride = NN;
            A.pk = dpk; A.lam0 = dl0; A.lam0_stride = 0; A.lam0_estride = n;
            A.a = da; A.P = dP; A.K = dK; A.lamT = dl1;
            A.status = fres; A.fail_t = fres + CF; A.skip = nullptr;
            AIY_TRY(launch_dist_forward_batch(A, c->st));
        }
        AIY_TRY(mark(2));
        {  // 3. E [m][T][N][Na] of economy i's base period-0 policy, read in place out of pk
            DistExpectArgs A{};
            A.N = (int)N; A.Na = (int)Na; A.C = (int)m; A.T = (int)T;
            A.pk = dpk; A.pk_stride = 3 * (size_t)T * n; A.y0 = dy; A.y0_stride = n;
            A.a = da; A.a_stride = (size_t)Na; A.P = dP; A.P_stride = NN; A.E = dE;
            AIY_TRY(launch_dist_expect_batch(A, c->st));
        }
        AIY_TRY(mark(3));
        {  // 4, 5. F and J [m][2][T][T]
            SsjFakeNewsArgs A{};
            A.T = (int)T; A.n_in = 2; A.n = (int)n; A.h = h; A.C = (int)m;
            A.E = dE; A.lam1 = dl1; A.F = dF; A.J = dJ;
            AIY_TRY(launch_ssj_fake_news(A, c->st));
        }
        AIY_TRY(mark(4));
        std::vector<int> hb(C3), hf(CF);
        for (int64_t i = 0; i < m; ++i) {
            const size_t o = (size_t)(e0 + i) * tt;
            AIY_TRY(c->down(J_r + o, dJ + 2 * i * tt, tt));
            AIY_TRY(c->down(J_w + o, dJ + (2 * i + 1) * tt, tt));
            if (F_r) AIY_TRY(c->down(F_r + o, dF + 2 * i * tt, tt));
            if (F_w) AIY_TRY(c->down(F_w + o, dF + (2 * i + 1) * tt, tt));
        }
        if (E) AIY_TRY(c->down(E + (size_t)e0 * T * n, dE, (size_t)m * T * n));
        AIY_TRY(c->down(hb.data(), bres, (size_t)C3));
        AIY_TRY(c->down(hf.data(), fres, (size_t)CF));
        AIY_TRY(c->sync());  // the next chunk reuses the buffers
        for (int64_t i = 0; i < m; ++i) {
            int sb = 0, sf = 0;
            for (int64_t p = 0; p < 3; ++p) sb |= hb[3 * i + p];
            for (int64_t p = 0; p < 3 * T; ++p) sf |= hf[3 * T * i + p];
            backward_status[e0 + i] = sb;
            forward_status[e0 + i] = sf;
            if (sb | sf) {  // a pass stopped: nothing downstream of it is a derivative
                double *jr = J_r + (size_t)(e0 + i) * tt, *jw = J_w + (size_t)(e0 + i) * tt;
                for (size_t q = 0; q < tt; ++q) jr[q] = jw[q] = nan;
            }
        }
        if (stage_ms)
            for (int q = 0; q < 4; ++q) {
                float ms = 0;
                AIY_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
                stage_ms[q] += ms;
            }
    }
    return AIY_OK;
}

int aiy_ssj_jacobian_labor(const double* policy_c, const double* lambda, double r_ss,
                           double w_ss, const double* a_grid, const double* s, const double* P,
                           int64_t N, int64_t Na, double beta, double sigma, double phi,
                           double theta, double amin, int64_t T, double h, double* J_Kr,
                           double* J_Kw, double* J_Hr, double* J_Hw, double* F_Kr, double* F_Kw,
                           double* F_Hr, double* F_Hw, double* E_a, double* E_h,
                           int32_t* backward_status, int32_t* forward_status, double* stage_ms) {
    if (!policy_c || !lambda || !s || !P || !J_Kr || !J_Kw || !J_Hr || !J_Hw ||
        !backward_status || !forward_status)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (!labor_egm_backward_fits(N, Na) || !labor_dist_forward_fits(N, Na))
        return fail(AIY_BAD_ARG, "Jacobian: the transition passes' arrays exceed one CU's LDS "
                                 "(aiy_labor_transition_batch's fit rules)");
    AIY_TRY(check_expect_shape(N, Na));
    AIY_TRY(check_fake_news(T, 2, N * Na, h));
    AIY_TRY(check_grid_strict(a_grid, Na));
    if (!std::isfinite(phi) || !(phi > 0))
        return fail(AIY_BAD_ARG, "phi must be positive and finite");
    if (!std::isfinite(theta) || theta == 0)
        return fail(AIY_BAD_ARG, "theta must be finite and not 0");
    if (!std::isfinite(r_ss) || !(1 + r_ss > 0) || !std::isfinite(r_ss + h))
        return fail(AIY_BAD_ARG, "r_ss must be finite with 1 + r_ss > 0");
    if (!std::isfinite(w_ss) || !std::isfinite(w_ss + h))
        return fail(AIY_BAD_ARG, "w_ss must be finite");
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    double *da, *ds, *dP;
    AIY_TRY(stage_common(c, a_grid, s, P, N, Na, &da, &ds, &dP));
    const size_t n = (size_t)N * Na, tt = (size_t)T * T;
    const int64_t C3 = 3, CF = 3 * T;
    // the three price paths: the steady state, r[T-1] + h, w[T-1] + h
    std::vector<double> rp(C3 * (T + 1), r_ss), wp(C3 * T, w_ss), y0(n);
    rp[(size_t)(T + 1) + T - 1] = r_ss + h;
    wp[2 * (size_t)T + T - 1] = w_ss + h;
    for (size_t e = 0; e < n; ++e) y0[e] = a_grid[e % Na];
    double *dr, *dw, *dc, *dl0, *dy, *dyh, *dpk, *dpl, *dK, *dH, *dl1, *dEa, *dEh, *dF, *dJ, *dG;
    int *bres, *fres;
    AIY_TRY(c->up_own("tr_r", std::move(rp), &dr));
    AIY_TRY(c->up_own("tr_w", std::move(wp), &dw));
    AIY_TRY(c->up_own("ssj_y0", std::move(y0), &dy));
    AIY_TRY(c->up("tr_pcT", policy_c, n, &dc));
    AIY_TRY(c->up("tr_l0", lambda, n, &dl0));
    AIY_TRY(c->room("ssj_yh", n, &dyh));
    AIY_TRY(c->room("tr_pk", (size_t)C3 * T * n, &dpk));
    AIY_TRY(c->room("tr_pl", (size_t)C3 * T * n, &dpl));
    AIY_TRY(c->room("tr_K", (size_t)CF * 2, &dK));
    AIY_TRY(c->room("tr_H", (size_t)CF, &dH));
    AIY_TRY(c->room("ssj_lam1", (size_t)CF * n, &dl1));
    AIY_TRY(c->room("ssj_E", (size_t)T * n, &dEa));
    AIY_TRY(c->room("ssj_Eh", (size_t)T * n, &dEh));
    AIY_TRY(c->room("ssj_F", 4 * tt, &dF));   // F_Kr, F_Kw, F_Hr, F_Hw
    AIY_TRY(c->room("ssj_J", 4 * tt, &dJ));   // J_Kr, J_Kw, J_Hr, J_Hw
    AIY_TRY(c->room("ssj_G", 2 * tt, &dG));
    AIY_TRY(c->room("ssj_bres", 2 * (size_t)C3, &bres));
    AIY_TRY(c->room("ssj_fres", 2 * (size_t)CF, &fres));
    Events ev;  // the stages' boundaries as the stream dispatches them
    if (stage_ms) AIY_TRY(ev.create(5, 0));
    auto mark = [&](int q) -> int {
        if (stage_ms) AIY_HIP(hipEventRecord(ev[q], c->st));
        return AIY_OK;
    };
    AIY_TRY(mark(0));
    {  // 1. the policies of an agent who learns of the change s periods ahead: pk, pl [3][T][N][Na]
        EgmBackwardArgs A{};
        A.N = (int)N; A.Na = (int)Na; A.C = (int)C3; A.T = (int)T;
        A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
        A.beta = beta; A.sigma = sigma; A.amin = amin; A.phi = phi; A.theta = theta;
        A.r = dr; A.w = dw; A.pcT = dc; A.pcT_stride = 0;
        A.a = da; A.s = ds; A.P = dP; A.pk = dpk; A.pl = dpl; A.pc = nullptr;
        A.status = bres; A.fail_t = bres + C3;
        AIY_TRY(launch_labor_egm_backward_batch(A, c->st));
    }
    AIY_TRY(mark(1));
    {  // 2. one push of the steady state's λ through each of them: Λ1 [3][T][N][Na], H1 [3][T]
        DistForwardArgs A{};
        A.N = (int)N; A.Na = (int)Na; A.C = (int)CF; A.T = 1;
        A.pk = dpk; A.pl = dpl; A.lam0 = dl0; A.lam0_stride = 0;
        A.a = da; A.s = ds; A.P = dP; A.K = dK; A.H = dH; A.lamT = dl1;
        A.status = fres; A.fail_t = fres + CF; A.skip = nullptr;
        AIY_TRY(launch_labor_dist_forward_batch(A, c->st));
    }
    AIY_TRY(mark(2));
    // 3. the expectation vectors of assets and of hours under the base path's period-0 policies
    AIY_TRY(launch_ssj_hours_outcome(ds, dpl, (int)N, (int)Na, dyh, c->st));
    AIY_TRY(expect_dev(N, Na, 1, T, dpk, dy, true, da, dP, dEa, c->st));
    AIY_TRY(expect_dev(N, Na, 1, T, dpk, dyh, true, da, dP, dEh, c->st));
    AIY_TRY(mark(3));
    // 4, 5. the fake-news matrices and the Jacobians: capital, then hours
    AIY_TRY(fake_news_dev(T, 2, (int64_t)n, dEa, dl1, h, dF, dJ, c->st));
    {
        SsjHoursArgs A{};
        A.T = (int)T; A.n_in = 2; A.n = (int)n; A.h = h;
        A.Eh = dEh; A.lam1 = dl1; A.H1 = dH; A.G = dG; A.F = dF + 2 * tt; A.J = dJ + 2 * tt;
        AIY_TRY(launch_ssj_hours_jacobian(A, c->st));
    }
    AIY_TRY(mark(4));
    std::vector<int> hb(C3), hf(CF);
    double* const Jo[4] = {J_Kr, J_Kw, J_Hr, J_Hw};
    double* const Fo[4] = {F_Kr, F_Kw, F_Hr, F_Hw};
    for (int q = 0; q < 4; ++q) {
        AIY_TRY(c->down(Jo[q], dJ + q * tt, tt));
        if (Fo[q]) AIY_TRY(c->down(Fo[q], dF + q * tt, tt));
    }
    if (E_a) AIY_TRY(c->down(E_a, dEa, (size_t)T * n));
    if (E_h) AIY_TRY(c->down(E_h, dEh, (size_t)T * n));
    AIY_TRY(c->down(hb.data(), bres, (size_t)C3));
    AIY_TRY(c->down(hf.data(), fres, (size_t)CF));
    AIY_TRY(c->sync());
    int sb = 0, sf = 0;
    for (int v : hb) sb |= v;
    for (int v : hf) sf |= v;
    *backward_status = sb;
    *forward_status = sf;
    if (sb | sf) {  // a pass stopped: nothing downstream of it is a derivative
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int q = 0; q < 4; ++q)
            for (size_t e = 0; e < tt; ++e) Jo[q][e] = nan;
    }
    if (stage_ms)
        for (int q = 0; q < 4; ++q) {
            float ms = 0;
            AIY_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            stage_ms[q] = ms;
        }
    return AIY_OK;
}

}  // extern "C"
