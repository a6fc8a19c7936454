// Estimation entry points: the MA coefficients of C shock processes (aiy_ssj_ma_batch[_dev]) and
// the autocovariances and Gaussian log-likelihoods of C candidates (aiy_ssj_loglik_batch[_dev]).
// Everything a host entry can refuse it refuses before it asks for a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "lik.hpp"

namespace aiy {

static int check_ma(int64_t n_o, int64_t T, int64_t C) {
    if (n_o < 1 || n_o > kLikMaxNo) return fail(AIY_BAD_SHAPE, "need 1 <= n_o <= 64");
    if (T < 1 || T > kSsjMaxT) return fail(AIY_BAD_SHAPE, "T must be in [1, 32768]");
    if (C < 1 || C > (1ll << 24)) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 2^24");
    return AIY_OK;
}

static int check_lik(int64_t C, int64_t n_o, int64_t T, int64_t L) {
    AIY_TRY(check_ma(n_o, T, C));
    if (L < 1) return fail(AIY_BAD_SHAPE, "need L >= 1");
    if (!lik_fits(n_o, L, T))
        return fail(AIY_BAD_ARG, "likelihood batch: a candidate's arrays exceed one CU's LDS "
                                 "(lik_fits: n = L·n_o, max(n(n+1)/2, n_o·T) + n·n_o + 3n + 2 "
                                 "doubles within 160 KiB)");
    return AIY_OK;
}

static int ma_dev(int64_t n_o, int64_t T, int64_t C, const double* G, const double* dZ, double* m,
                  hipStream_t st) {
    SsjMaArgs A{};
    A.n_o = (int)n_o; A.T = (int)T; A.C = (int)C;
    A.G = G; A.dZ = dZ; A.m = m;
    return launch_ssj_ma_batch(A, st);
}

static int lik_dev(int64_t C, int64_t n_o, int64_t T, int64_t L, const double* m, const double* y,
                   const double* me_var, bool shared, double* loglik, int* status, int* fail_j,
                   double* Gamma, double* d, hipStream_t st) {
    SsjLikArgs A{};
    A.C = (int)C; A.n_o = (int)n_o; A.T = (int)T; A.L = (int)L;
    A.m = m; A.y = y; A.me_var = me_var;
    A.me_stride = shared ? 0 : (size_t)n_o;
    A.loglik = loglik; A.status = status; A.fail = fail_j; A.Gamma = Gamma; A.d = d;
    return launch_ssj_loglik_batch(A, st);
}

// with y: me_var and the three result arrays are needed; without: Gamma is the only result
static int check_lik_ptrs(const double* m, const double* y, const double* me_var,
                          const double* loglik, const int32_t* status, const int32_t* fail_j,
                          const double* Gamma) {
    if (!m) return fail(AIY_BAD_ARG, "NULL argument");
    if (y ? (!me_var || !loglik || !status || !fail_j) : !Gamma)
        return fail(AIY_BAD_ARG, "NULL argument");
    return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_ssj_ma_batch_dev(int64_t n_o, int64_t T, int64_t C, const double* G, const double* dZ,
                         double* m, void* stream) {
    if (!G || !dZ || !m) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_ma(n_o, T, C));
    return ma_dev(n_o, T, C, G, dZ, m, (hipStream_t)stream);
}

int aiy_ssj_ma_batch(int64_t n_o, int64_t T, int64_t C, const double* G, const double* dZ,
                     double* m) {
    if (!G || !dZ || !m) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_ma(n_o, T, C));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(1, 2, 1, &c));
    const size_t gt = (size_t)n_o * T * T, zt = (size_t)C * T, mt = (size_t)C * n_o * T;
    double *dG, *dz, *dm;
    AIY_TRY(c->up("lik_G", G, gt, &dG));
    AIY_TRY(c->up("lik_dZ", dZ, zt, &dz));
    AIY_TRY(c->room("lik_m", mt, &dm));
    AIY_TRY(ma_dev(n_o, T, C, dG, dz, dm, c->st));
    AIY_TRY(c->down(m, dm, mt));
    return c->sync();
}

int aiy_ssj_loglik_batch_dev(int64_t C, int64_t n_o, int64_t T, int64_t L, const double* m,
                             const double* y, const double* me_var, int me_var_shared,
                             double* loglik, int32_t* status, int32_t* fail_j, double* Gamma,
                             double* d, void* stream) {
    AIY_TRY(check_lik_ptrs(m, y, me_var, loglik, status, fail_j, Gamma));
    AIY_TRY(check_lik(C, n_o, T, L));
    return lik_dev(C, n_o, T, L, m, y, me_var, me_var_shared != 0, loglik, status, fail_j, Gamma,
                   d, (hipStream_t)stream);
}

int aiy_ssj_loglik_batch(int64_t C, int64_t n_o, int64_t T, int64_t L, const double* m,
                         const double* y, const double* me_var, int me_var_shared, double* loglik,
                         int32_t* status, int32_t* fail_j, double* Gamma, double* d) {
    AIY_TRY(check_lik_ptrs(m, y, me_var, loglik, status, fail_j, Gamma));
    AIY_TRY(check_lik(C, n_o, T, L));
    const size_t nme = y ? (size_t)n_o * (me_var_shared ? 1 : (size_t)C) : 0;
    for (size_t q = 0; q < nme; ++q)
        if (!(me_var[q] >= 0) || !std::isfinite(me_var[q]))
            return fail(AIY_BAD_ARG, "me_var must be finite and >= 0 (entry %lld)",
                        (long long)q + 1);
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(1, 2, 1, &c));
    const size_t n = (size_t)n_o * L, mt = (size_t)C * n_o * T, gt = (size_t)C * n * n_o;
    double *dm, *dy = nullptr, *dme = nullptr, *dll = nullptr, *dG = nullptr, *dd = nullptr;
    int *dst = nullptr, *dfl = nullptr;
    AIY_TRY(c->up("lik_m", m, mt, &dm));
    if (y) {
        AIY_TRY(c->up("lik_y", y, n, &dy));
        AIY_TRY(c->up("lik_me", me_var, nme, &dme));
        AIY_TRY(c->room("lik_ll", (size_t)C, &dll));
        AIY_TRY(c->room("lik_st", (size_t)C, &dst));
        AIY_TRY(c->room("lik_fl", (size_t)C, &dfl));
        if (d) AIY_TRY(c->room("lik_d", (size_t)C * n, &dd));
    }
    if (Gamma) AIY_TRY(c->room("lik_Gam", gt, &dG));
    AIY_TRY(lik_dev(C, n_o, T, L, dm, dy, dme, me_var_shared != 0, dll, dst, dfl, dG, dd, c->st));
    if (y) {
        AIY_TRY(c->down(loglik, dll, (size_t)C));
        AIY_TRY(c->down(status, dst, (size_t)C));
        AIY_TRY(c->down(fail_j, dfl, (size_t)C));
        if (d) AIY_TRY(c->down(d, dd, (size_t)C * n));
    }
    if (Gamma) AIY_TRY(c->down(Gamma, dG, gt));
    return c->sync();
}

}  // extern "C"
