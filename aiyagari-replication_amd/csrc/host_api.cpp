// Host tier of the C ABI: MATLAB column-major arrays in and out, synchronous.  Each call
// stages its inputs into library-owned device buffers (cached per shape), runs the device
// tier and copies the outputs back in the layout of the variables the call replaces.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "ws.hpp"

namespace aiy {

static std::mutex g_mu;
static std::map<std::tuple<int, int64_t, int64_t, int64_t>, std::unique_ptr<HostCtx>> g_ctx;

HostCtx::~HostCtx() {
    bufs.m.clear();  // the buffers first, then the workspace and the stream they were used on
    if (ws) aiy_ws_destroy(ws);
    if (st) (void)hipStreamDestroy(st);
}

int get_ctx(int64_t N, int64_t Na, int64_t Nl, HostCtx** out) {
    int dev = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AIY_NO_DEVICE, "no HIP device visible");
    (void)hipGetDevice(&dev);
    auto key = std::make_tuple(dev, N, Na, Nl);
    auto it = g_ctx.find(key);
    if (it != g_ctx.end()) {
        *out = it->second.get();
        return AIY_OK;
    }
    auto ctx = std::make_unique<HostCtx>();
    AIY_TRY(aiy_ws_create(N, Na, Nl, &ctx->ws));
    AIY_HIP(hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking));
    *out = ctx.get();
    g_ctx[key] = std::move(ctx);
    return AIY_OK;
}

std::mutex& host_mutex() { return g_mu; }

int check_grid(const double* a, int64_t Na) {
    if (!a) return fail(AIY_BAD_ARG, "a_grid is NULL");
    for (int64_t k = 0; k < Na; ++k)
        if (!std::isfinite(a[k])) return fail(AIY_NON_FINITE, "a_grid(%lld) is not finite", (long long)k + 1);
    for (int64_t k = 1; k < Na; ++k)
        if (a[k] < a[k - 1])
            return fail(AIY_BAD_ARG, "a_grid must be non-decreasing (a_grid(%lld) < a_grid(%lld))",
                        (long long)k + 1, (long long)k);
    return AIY_OK;
}

// interp1 and griddedInterpolant reject repeated grid points: the interpolating entry points
// (simulation, histogram lottery, KS panel) need a strictly increasing grid, else they would
// divide by a[k+1] - a[k] = 0 (MATLAB raises an error there)
int check_grid_strict(const double* a, int64_t Na) {
    AIY_TRY(check_grid(a, Na));
    for (int64_t k = 1; k < Na; ++k)
        if (!(a[k] > a[k - 1]))
            return fail(AIY_BAD_ARG, "grid must be strictly increasing (point %lld repeats point %lld)",
                        (long long)k + 1, (long long)k);
    return AIY_OK;
}

// stage the common Aiyagari inputs (a_grid, s, P) on the device; P transposed to row-major
int stage_common(HostCtx* c, const double* a, const double* s, const double* P, int64_t N,
                 int64_t Na, double** da, double** ds, double** dP) {
    AIY_TRY(c->up("a", a, (size_t)Na, da));
    AIY_TRY(c->up("s", s, (size_t)N, ds));
    AIY_TRY(c->up_rows("P", P, N, N, 1, dP));
    AIY_TRY(c->sync());
    aiy_ws_invalidate(c->ws);  // the staged a/s contents may differ from the last call
    return AIY_OK;
}

std::vector<int> idx_rows0(const int32_t* idx1, int vfi_layout, int64_t N, int64_t Na, int64_t C) {
    const size_t n = (size_t)N * Na;
    std::vector<int> out(n * (size_t)C, 0);
    if (!idx1) return out;
    if (vfi_layout)
        for (int64_t q = 0; q < C; ++q) cm_to_rows(idx1 + q * n, N, Na, out.data() + q * n);
    else
        out.assign(idx1, idx1 + out.size());
    for (int& k : out) k -= 1;
    return out;
}

// The host body of the four VFI entries, arrays N x Na column-major.  Aiyagari_VFI.m (!labor):
// v_new and the policies are outputs only and are never read.  The labour script (A3): they
// are in/out — a state without a feasible choice keeps what came in — so they go up first.
static int vfi_host(bool labor, const double* v_old_cm, const double* a, const double* s,
                    const double* P, const double* L, int64_t N, int64_t Na, int64_t Nl, double r,
                    double w, double beta, double sigma, double psi, double eta, bool solve,
                    double tol, int64_t max_iter, double* v_old_out_cm, double* v_new_cm,
                    double* pk_cm, double* pl_cm, double* pc_cm, int32_t* idx_cm, int64_t* iters) {
    if (!v_old_cm || !s || !P || !v_new_cm || !pk_cm || !pc_cm || (labor && (!L || !pl_cm)))
        return fail(AIY_BAD_ARG, "NULL argument");
    if (labor && (N < 1 || Na < 2 || Nl < 1))
        return fail(AIY_BAD_SHAPE, "need N >= 1, Na >= 2, Nl >= 1");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    AIY_TRY(check_grid(a, Na));
    std::lock_guard<std::mutex> lk(g_mu);
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, Nl, &c));
    const size_t n = (size_t)N * Na;
    double *da, *ds, *dP, *dva, *dvb, *dpk, *dpc, *dpl = nullptr, *dL = nullptr;
    int* didx;
    AIY_TRY(stage_common(c, a, s, P, N, Na, &da, &ds, &dP));
    AIY_TRY(c->up_rows("va", v_old_cm, N, Na, 1, &dva));
    if (labor) {
        AIY_TRY(c->up_rows("vb", v_new_cm, N, Na, 1, &dvb));
        AIY_TRY(c->up_rows("pk", pk_cm, N, Na, 1, &dpk));
        AIY_TRY(c->up_rows("pl", pl_cm, N, Na, 1, &dpl));
        AIY_TRY(c->up_rows("pc", pc_cm, N, Na, 1, &dpc));
        AIY_TRY(c->up_own("idx", idx_rows0(idx_cm, 1, N, Na), &didx));
        AIY_TRY(c->up("L", L, (size_t)Nl, &dL));
    } else {
        AIY_TRY(c->room("vb", n, &dvb));
        AIY_TRY(c->room("pk", n, &dpk));
        AIY_TRY(c->room("pc", n, &dpc));
        AIY_TRY(c->room("idx", n, &didx));
    }
    int out_new = 1;
    BellCall bc{};
    if (labor) {
        bc.labor = true; bc.Nl = Nl; bc.L = dL; bc.psi = psi; bc.eta = eta;
    }
    bc.a = da; bc.s = ds; bc.P = dP; bc.r = r; bc.w = w; bc.beta = beta; bc.sigma = sigma;
    bc.idx = didx; bc.pk = dpk; bc.pl = dpl; bc.pc = dpc;
    if (solve) {
        // the MATLAB labour loop keeps v_new across sweeps; at sweep 1 the ping-pong partner of
        // v_old must hold the incoming v_new, which merge copies from v_old where needed
        AIY_TRY(bell_solve_dev(c->ws, bc, dva, dvb, tol, max_iter, iters, &out_new, c->st));
    } else {
        bc.v_old = dva;
        bc.v_new = dvb;
        AIY_TRY(bell_sweep_dev(c->ws, bc, c->st));
    }
    AIY_TRY(c->down_rows(v_new_cm, out_new ? dvb : dva, N, Na, 1));
    AIY_TRY(c->down_rows(pk_cm, dpk, N, Na, 1));
    if (labor) AIY_TRY(c->down_rows(pl_cm, dpl, N, Na, 1));
    AIY_TRY(c->down_rows(pc_cm, dpc, N, Na, 1));
    if (solve && v_old_out_cm) AIY_TRY(c->down_rows(v_old_out_cm, out_new ? dva : dvb, N, Na, 1));
    if (idx_cm) {  // back to MATLAB's 1-based index
        AIY_TRY(c->down_rows(idx_cm, didx, N, Na, 1));
        for (size_t k = 0; k < n; ++k) idx_cm[k] += 1;
    }
    return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_release_all(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& kv : g_ctx) {  // each context's buffers live on its own device
        (void)hipSetDevice(std::get<0>(kv.first));
        kv.second.reset();
    }
    g_ctx.clear();
    (void)hipSetDevice(cur);
    return AIY_OK;
}

int64_t aiy_host_cache_bytes(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int64_t b = 0;
    for (auto& kv : g_ctx) b += (int64_t)kv.second->bufs.bytes();
    return b;
}

int aiy_vfi_sweep(const double* v_old, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double* v_new, double* policy_k, double* policy_c, int32_t* policy_idx) {
    return vfi_host(false, v_old, a_grid, s, P, nullptr, N, Na, 1, r, w, beta, sigma, 0, 0, false,
                    0, 1, nullptr, v_new, policy_k, nullptr, policy_c, policy_idx, nullptr);
}

int aiy_vfi_solve(double* v_old, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double tol, int64_t max_iter, double* v_new, double* policy_k,
                  double* policy_c, int32_t* policy_idx, int64_t* iters) {
    if (!iters) return fail(AIY_BAD_ARG, "NULL iters");
    return vfi_host(false, v_old, a_grid, s, P, nullptr, N, Na, 1, r, w, beta, sigma, 0, 0, true,
                    tol, max_iter, v_old, v_new, policy_k, nullptr, policy_c, policy_idx, iters);
}

int aiy_labor_vfi_sweep(const double* v_old, const double* a_grid, const double* s,
                        const double* P, const double* labor_choice, int64_t N, int64_t Na,
                        int64_t Nl, double r, double w, double beta, double sigma, double psi,
                        double eta, double* v_new, double* policy_k, double* policy_l,
                        double* policy_c, int32_t* policy_lin) {
    return vfi_host(true, v_old, a_grid, s, P, labor_choice, N, Na, Nl, r, w, beta, sigma, psi,
                    eta, false, 0, 1, nullptr, v_new, policy_k, policy_l, policy_c, policy_lin,
                    nullptr);
}

int aiy_labor_vfi_solve(double* v_old, const double* a_grid, const double* s, const double* P,
                        const double* labor_choice, int64_t N, int64_t Na, int64_t Nl, double r,
                        double w, double beta, double sigma, double psi, double eta, double tol,
                        int64_t max_iter, double* v_new, double* policy_k, double* policy_l,
                        double* policy_c, int32_t* policy_lin, int64_t* iters) {
    if (!iters) return fail(AIY_BAD_ARG, "NULL iters");
    return vfi_host(true, v_old, a_grid, s, P, labor_choice, N, Na, Nl, r, w, beta, sigma, psi,
                    eta, true, tol, max_iter, v_old, v_new, policy_k, policy_l, policy_c, policy_lin,
                    iters);
}

}  // extern "C"
