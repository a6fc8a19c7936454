// F2 histogram entry points: ks_simulate_hist (MATLAB layouts, synchronous) and its device tier
// ks_simulate_hist_dev.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "ks_hist.hpp"
#include "ks_panel.hpp"

namespace aiy {

static int check_hist_shape(int64_t nk, int64_t nK, int64_t nx, int64_t T, int64_t M) {
    if (T < 2 || T > (1ll << 30)) return fail(AIY_BAD_SHAPE, "T must be in [2, 2^30]");
    if (M < 1 || M > kHistMaxPaths) return fail(AIY_BAD_SHAPE, "need 1 <= M <= 65,535 shock paths");
    if (!ks_hist_fits(nx, nk, nK))
        return fail(AIY_BAD_SHAPE,
                    "histogram simulation: need nx, k_size, K_size >= 2 and a path's state "
                    "inside one CU's LDS: 8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB");
    return AIY_OK;
}

static int check_hist_params(const double* params) {
    for (int q = 0; q < 13; ++q)
        if (!std::isfinite(params[q])) return fail(AIY_NON_FINITE, "non-finite params");
    const double ug = params[5], ub = params[6];
    if (!(ug > 0 && ug < 1 && ub > 0 && ub < 1))
        return fail(AIY_BAD_ARG, "ug and ub must lie in (0, 1)");
    return AIY_OK;
}

// What both tiers pass: the single tier adds thr (by value), the multi tier pol and thr_g.
static HistArgs hist_args(int64_t nk, int64_t nK, const double* k_grid, const double* K_grid,
                          const double* k_opt, const double* x_grid, int64_t nx, const int8_t* zi,
                          int64_t T, int64_t M, double* lam, double* K_ts, int64_t* slow) {
    HistArgs A{};
    A.nx = (int)nx;
    A.nk = (int)nk;
    A.nK = (int)nK;
    A.T = (int)T;
    A.M = (int)M;
    A.k_grid = k_grid;
    A.K_grid = K_grid;
    A.x = x_grid;
    A.k_opt = k_opt;
    A.zi = zi;
    A.lam = lam;
    A.K_ts = K_ts;
    A.slow = slow;
    return A;
}

int hist_dev(int64_t nk, int64_t nK, const double* k_grid, const double* K_grid,
             const double* k_opt, const double* x_grid, int64_t nx, const double* params,
             const int8_t* zi, int64_t T, int64_t M, double* lam, double* K_ts, int64_t* slow,
             hipStream_t st) {
    if (!k_grid || !K_grid || !k_opt || !x_grid || !params || !zi || !lam || !K_ts)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_hist_shape(nk, nK, nx, T, M));
    AIY_TRY(check_hist_params(params));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AIY_NO_DEVICE, "no HIP device visible");
    ShockArgs S{};
    shock_probs(params[5], params[6], S);
    HistArgs A = hist_args(nk, nK, k_grid, K_grid, k_opt, x_grid, nx, zi, T, M, lam, K_ts, slow);
    for (int q = 0; q < 8; ++q) A.thr[q] = S.thr[q];
    return launch_ks_hist(A, st);
}

// ---- one policy per path.  Device scratch of a call: thr [C][8] doubles, then pol [M] int32.
static size_t hist_multi_scratch(int64_t C, int64_t M) {
    return sizeof(double) * 8 * (size_t)C + sizeof(int32_t) * (size_t)M;
}

static int check_hist_multi(int64_t C, const double* params, const int32_t* pol, int64_t M) {
    if (C < 1 || C > kHistMaxPaths) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 65,535 candidates");
    for (int64_t c = 0; c < C; ++c) AIY_TRY(check_hist_params(params + 13 * c));
    for (int64_t m = 0; m < M; ++m)
        if (pol[m] < 0 || pol[m] >= C)
            return fail(AIY_BAD_ARG, "policy_of_path(%lld) = %d is outside [0, C)",
                        (long long)(m + 1), (int)pol[m]);
    return AIY_OK;
}

// k_grid, K_grid [C][nK], k_opt [C][4][nK][nk], x_grid, zi, lam, K_ts, slow and scratch on the
// device; params [C][13] and pol [M] on the host (validated by the caller).  The tables are
// uploaded on `st` and the call waits for that copy before they die; the launch is left running.
static int hist_multi_dev(int64_t C, int64_t nk, int64_t nK, const double* k_grid,
                          const double* K_grid, const double* k_opt, const double* x_grid,
                          int64_t nx, const double* params, const int32_t* pol, const int8_t* zi,
                          int64_t T, int64_t M, double* lam, double* K_ts, int64_t* slow,
                          void* scratch, hipStream_t st) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AIY_NO_DEVICE, "no HIP device visible");
    std::vector<double> thr(8 * (size_t)C);
    for (int64_t c = 0; c < C; ++c) {
        ShockArgs S{};
        shock_probs(params[13 * c + 5], params[13 * c + 6], S);
        for (int q = 0; q < 8; ++q) thr[8 * c + q] = S.thr[q];
    }
    double* dthr = (double*)scratch;
    int32_t* dpol = (int32_t*)(dthr + 8 * C);
    AIY_HIP(hipMemcpyAsync(dthr, thr.data(), sizeof(double) * thr.size(), hipMemcpyHostToDevice, st));
    AIY_HIP(hipMemcpyAsync(dpol, pol, sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
    AIY_HIP(hipStreamSynchronize(st));
    HistArgs A = hist_args(nk, nK, k_grid, K_grid, k_opt, x_grid, nx, zi, T, M, lam, K_ts, slow);
    A.pol = dpol;
    A.thr_g = dthr;
    return launch_ks_hist(A, st);
}

// The host-tier body of ks_simulate_hist (pol == nullptr: one policy, C = 1, buffers ksh_*) and
// ks_simulate_hist_multi (pol [M], C candidates, buffers kshm_*), behind their own checks: the
// validated inputs up, the entry's device tier, lam, K_ts and the slow-period counts back.
static int hist_host(int64_t C, const double* k_opt, const double* k_grid, const double* K_grid,
                     int64_t nk, int64_t nK, const double* x_grid, int64_t nx,
                     const double* params, const int32_t* pol, const std::vector<int8_t>& hz,
                     int64_t T, int64_t M, double* lam, double* K_ts, int64_t* slow_periods) {
    const size_t nko = (size_t)C * nk * nK * 4, nl = (size_t)2 * nx * M, nz = (size_t)T * M;
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(4 * nK, nk, 1, &c));
    const std::string pre = pol ? "kshm_" : "ksh_";
    auto nm = [&](const char* s) { return pre + s; };
    double *dko, *dkg, *dKg, *dx, *dlam, *dKts;
    int64_t* dslow;
    int8_t* dz;
    AIY_TRY(c->up(nm("kopt").c_str(), k_opt, nko, &dko));
    AIY_TRY(c->up(nm("kg").c_str(), k_grid, nk, &dkg));
    AIY_TRY(c->up(nm("Kg").c_str(), K_grid, C * nK, &dKg));
    AIY_TRY(c->up(nm("x").c_str(), x_grid, nx, &dx));
    AIY_TRY(c->up(nm("lam").c_str(), lam, nl, &dlam));
    AIY_TRY(c->room(nm("Kts").c_str(), nz, &dKts));
    AIY_TRY(c->room(nm("slow").c_str(), M, &dslow));
    AIY_TRY(c->up(nm("zi").c_str(), hz.data(), nz, &dz));
    if (pol) {
        unsigned char* dscr;
        AIY_TRY(c->room("kshm_scratch", hist_multi_scratch(C, M), &dscr));
        AIY_TRY(hist_multi_dev(C, nk, nK, dkg, dKg, dko, dx, nx, params, pol, dz, T, M, dlam,
                               dKts, dslow, dscr, c->st));
    } else {
        AIY_TRY(hist_dev(nk, nK, dkg, dKg, dko, dx, nx, params, dz, T, M, dlam, dKts, dslow,
                         c->st));
    }
    AIY_TRY(c->down(lam, dlam, nl));
    AIY_TRY(c->down(K_ts, dKts, nz));
    std::vector<int64_t> hs(M);
    AIY_TRY(c->down(hs.data(), dslow, M));
    AIY_HIP(hipStreamSynchronize(c->st));
    if (slow_periods)
        for (int64_t m = 0; m < M; ++m) slow_periods[m] = hs[m];
    return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int64_t ks_hist_multi_scratch_bytes(int64_t C, int64_t M) {
    return (C < 1 || M < 1) ? 0 : (int64_t)hist_multi_scratch(C, M);
}

int ks_simulate_hist_multi_dev(int64_t C, int64_t nk, int64_t nK, const double* k_grid,
                               const double* K_grid, const double* k_opt, const double* x_grid,
                               int64_t nx, const double* params, const int32_t* policy_of_path,
                               const int8_t* zi, int64_t T, int64_t M, double* lam, double* K_ts,
                               int64_t* slow_periods, void* scratch, void* stream) {
    if (!k_grid || !K_grid || !k_opt || !x_grid || !params || !policy_of_path || !zi || !lam ||
        !K_ts || !scratch)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_hist_shape(nk, nK, nx, T, M));
    AIY_TRY(check_hist_multi(C, params, policy_of_path, M));
    return hist_multi_dev(C, nk, nK, k_grid, K_grid, k_opt, x_grid, nx, params, policy_of_path, zi,
                          T, M, lam, K_ts, slow_periods, scratch, (hipStream_t)stream);
}

int ks_simulate_hist_multi(int64_t C, const double* k_opt, const double* k_grid,
                           const double* K_grid, int64_t nk, int64_t nK, const double* x_grid,
                           int64_t nx, const double* params, const int32_t* policy_of_path,
                           const double* zi_shock, int64_t T, int64_t M, double* lam,
                           double* K_ts, int64_t* slow_periods) {
    if (!k_opt || !k_grid || !K_grid || !x_grid || !params || !policy_of_path || !zi_shock ||
        !lam || !K_ts)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_hist_shape(nk, nK, nx, T, M));
    AIY_TRY(check_hist_multi(C, params, policy_of_path, M));
    AIY_TRY(check_grid_strict(k_grid, nk));  // all three are interpolated
    for (int64_t c = 0; c < C; ++c) AIY_TRY(check_grid_strict(K_grid + c * nK, nK));
    AIY_TRY(check_grid_strict(x_grid, nx));
    const size_t nko = (size_t)C * nk * nK * 4, nl = (size_t)2 * nx * M, nz = (size_t)T * M;
    for (size_t q = 0; q < nko; ++q)
        if (!std::isfinite(k_opt[q])) return fail(AIY_NON_FINITE, "non-finite k_opt");
    for (size_t q = 0; q < nl; ++q)
        if (!std::isfinite(lam[q])) return fail(AIY_NON_FINITE, "non-finite lam");
    std::vector<int8_t> hz;
    AIY_TRY(zi_to_i8(zi_shock, nz, hz));
    return hist_host(C, k_opt, k_grid, K_grid, nk, nK, x_grid, nx, params, policy_of_path, hz, T,
                     M, lam, K_ts, slow_periods);
}

int ks_simulate_hist_dev(int64_t nk, int64_t nK, const double* k_grid, const double* K_grid,
                         const double* k_opt, const double* x_grid, int64_t nx,
                         const double* params, const int8_t* zi, int64_t T, int64_t M,
                         double* lam, double* K_ts, int64_t* slow_periods, void* stream) {
    return hist_dev(nk, nK, k_grid, K_grid, k_opt, x_grid, nx, params, zi, T, M, lam, K_ts,
                    slow_periods, (hipStream_t)stream);
}

int ks_simulate_hist(const double* k_opt, const double* k_grid, const double* K_grid, int64_t nk,
                     int64_t nK, const double* x_grid, int64_t nx, const double* params,
                     const double* zi_shock, int64_t T, int64_t M, double* lam, double* K_ts,
                     int64_t* slow_periods) {
    if (!k_opt || !k_grid || !K_grid || !x_grid || !params || !zi_shock || !lam || !K_ts)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_hist_shape(nk, nK, nx, T, M));
    AIY_TRY(check_grid_strict(k_grid, nk));  // all three are interpolated
    AIY_TRY(check_grid_strict(K_grid, nK));
    AIY_TRY(check_grid_strict(x_grid, nx));
    AIY_TRY(check_hist_params(params));
    const size_t nko = (size_t)nk * nK * 4, nl = (size_t)2 * nx * M, nz = (size_t)T * M;
    for (size_t q = 0; q < nko; ++q)
        if (!std::isfinite(k_opt[q])) return fail(AIY_NON_FINITE, "non-finite k_opt");
    for (size_t q = 0; q < nl; ++q)
        if (!std::isfinite(lam[q])) return fail(AIY_NON_FINITE, "non-finite lam");
    // T x M column-major: path m's chain is contiguous, the device tier's [M][T]
    std::vector<int8_t> hz;
    AIY_TRY(zi_to_i8(zi_shock, nz, hz));
    return hist_host(1, k_opt, k_grid, K_grid, nk, nK, x_grid, nx, params, nullptr, hz, T, M, lam,
                     K_ts, slow_periods);
}

}  // extern "C"
