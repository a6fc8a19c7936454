// C ABI (include/aiyagari_hip.h): error reporting, workspace management and the Bellman
// device-tier entries (their drivers: bell_host.cpp).  Host code only; kernels live in
// *_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <string>
#include <thread>
#include <vector>

#include "aiy_common.hpp"
#include "ws.hpp"

namespace aiy {

int wait_event(hipEvent_t ev) {
    for (int spin = 0;; ++spin) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return AIY_OK;
        if (e != hipErrorNotReady) {
            (void)hipGetLastError();
            return fail(AIY_HIP_ERROR, "hipEventQuery failed: %s", hipGetErrorString(e));
        }
        if (spin > 256) std::this_thread::yield();
    }
}

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ---------------------------------------------------------------------------- workspace
int ws_ensure_diff(aiy_ws* ws) {
    AIY_TRY(ws->diff.ensure(2 * kDiffSlots));
    return ws->hdiff.ensure(2 * kDiffSlots + 4);
}

int ws_ensure_trace(aiy_ws* ws, int64_t units, bool* fresh) {
    return ws->trace.ensure(16 * (size_t)units, fresh);
}

int ws_ensure_bell(aiy_ws* ws, size_t partial_slots) {
    const size_t n = (size_t)ws->N * ws->Na;
    bool fresh;
    AIY_TRY(ws->EV.ensure(n));
    AIY_TRY(ws->T.ensure(n));
    AIY_TRY(ws->T32.ensure(2 * (size_t)ws->N * (ws->Na + (ws->Na & 1))));
    AIY_TRY(ws->Dm.ensure((size_t)ws->N * ((ws->Na + 63) / 64)));
    AIY_TRY(ws->Dm8.ensure((size_t)ws->N * ((ws->Na + 7) / 8)));
    AIY_TRY(ws->Dt.ensure(n));
    AIY_TRY(ws->Dm512.ensure((size_t)ws->N * ((ws->Na + 511) / 512)));
    AIY_TRY(ws->best0.ensure(n));
    AIY_TRY(ws->idx0.ensure(n));
    AIY_TRY(ws->mom.ensure(n, &fresh));
    if (fresh) AIY_HIP(hipMemset(ws->mom, 0, n * sizeof(int)));
    AIY_TRY(ws->touched.ensure(n, &fresh));  // the merge kernel leaves touched = 0 and
    if (fresh) AIY_HIP(hipMemset(ws->touched, 0, n * sizeof(int)));  // partial = -1 behind
    AIY_TRY(ws->partial.ensure(partial_slots, &fresh));
    if (fresh) AIY_HIP(hipMemset(ws->partial, 0xff, partial_slots * sizeof(int)));
    AIY_TRY(ws_ensure_diff(ws));  // (here: the device allocations keep the order they always had)
    AIY_TRY(ws->hitcount.ensure(kHitcountLen, &fresh));
    if (fresh)  // zero from the start: counting may be switched on before a sweep
        AIY_HIP(hipMemset(ws->hitcount, 0, kHitcountLen * sizeof(unsigned long long)));
    return ws->dis.ensure((size_t)std::max<int64_t>(ws->Nl, 1));
}

int ws_timing_begin(aiy_ws* ws, hipStream_t st) {
    if (!ws->timing) return AIY_OK;
    if (ws->ev_used == (int)ws->ev_start.size()) AIY_TRY(ws_timing_drain(ws));
    AIY_HIP(hipEventRecord(ws->ev_start[ws->ev_used], st));
    return AIY_OK;
}
int ws_timing_end(aiy_ws* ws, hipStream_t st) {
    if (!ws->timing) return AIY_OK;
    AIY_HIP(hipEventRecord(ws->ev_stop[ws->ev_used], st));
    ws->ev_used++;
    return AIY_OK;
}
// dispatch-recorded events (dispatch.hpp) for the next timed launch on this thread; call
// ws_dispatch_commit after the launch whatever it returned
int ws_dispatch_arm(aiy_ws* ws) {
    if (!ws->timing) return AIY_OK;
    if (ws->ev_used == (int)ws->ev_start.size()) AIY_TRY(ws_timing_drain(ws));
    g_dispatch_ev = DispatchEvents{ws->ev_start[ws->ev_used], ws->ev_stop[ws->ev_used]};
    return AIY_OK;
}
void ws_dispatch_commit(aiy_ws* ws) {
    if (!ws->timing) return;
    if (!g_dispatch_ev.start) ws->ev_used++;  // the launch consumed (recorded) them
    g_dispatch_ev = DispatchEvents{};
}
int ws_timing_drain(aiy_ws* ws) {
    for (int q = 0; q < ws->ev_used; ++q) {
        AIY_HIP(hipEventSynchronize(ws->ev_stop[q]));
        float ms = 0.f;
        AIY_HIP(hipEventElapsedTime(&ms, ws->ev_start[q], ws->ev_stop[q]));
        ws->tot_ms += ms;
        ws->launches++;
    }
    ws->ev_used = 0;
    return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

// ============================================================================ C ABI
extern "C" {

const char* aiy_last_error(void) { return g_err.c_str(); }
int aiy_version(void) { return 100; }
int aiy_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int aiy_ws_create(int64_t N, int64_t Na, int64_t Nl, aiy_ws** out) {
    if (!out) return fail(AIY_BAD_ARG, "NULL out pointer");
    if (N < 1 || Na < 2 || N > (1 << 16) || Na > (1 << 28) || N * Na > (1ll << 31) - 1)
        return fail(AIY_BAD_SHAPE, "unsupported shape N=%lld Na=%lld", (long long)N,
                    (long long)Na);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AIY_NO_DEVICE, "no HIP device visible");
    aiy_ws* ws = new aiy_ws();
    ws->N = N;
    ws->Na = Na;
    ws->Nl = Nl < 1 ? 1 : Nl;
    (void)hipGetDevice(&ws->dev);
    if (ws->ev_start.create(64, 0) != AIY_OK || ws->ev_stop.create(64, 0) != AIY_OK) {
        delete ws;
        return AIY_HIP_ERROR;
    }
    *out = ws;
    return AIY_OK;
}

int aiy_ws_destroy(aiy_ws* ws) {
    delete ws;
    return AIY_OK;
}

int aiy_ws_set_timing(aiy_ws* ws, int enable) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    AIY_TRY(ws_timing_drain(ws));
    ws->timing = (enable & 1) != 0;
    ws->count_hits = (enable & 2) != 0;
    ws->tracing = (enable & 4) != 0;
    ws->tot_ms = 0;
    ws->launches = 0;
    if (ws->hitcount) AIY_HIP(hipMemset(ws->hitcount, 0, kHitcountLen * sizeof(unsigned long long)));
    if (ws->tracing && ws->trace)  // records of an earlier geometry must not linger
        AIY_HIP(hipMemset(ws->trace, 0, ws->trace.cap() * sizeof(long long)));
    return AIY_OK;
}

int aiy_ws_timing(aiy_ws* ws, double* total_ms, int64_t* launches, int64_t* hits) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    AIY_TRY(ws_timing_drain(ws));
    if (total_ms) *total_ms = ws->tot_ms;
    if (launches) *launches = ws->launches;
    if (hits) {
        int64_t c[4];
        AIY_TRY(aiy_ws_counters(ws, c));
        *hits = c[0];
    }
    return AIY_OK;
}

int aiy_ws_counters(aiy_ws* ws, int64_t out[4]) {
    if (!ws || !out) return fail(AIY_BAD_ARG, "NULL workspace/out");
    std::vector<unsigned long long> h(4 * kDiffSlots, 0ull);
    if (ws->hitcount)
        AIY_HIP(hipMemcpy(h.data(), ws->hitcount, h.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
    for (int q = 0; q < 4; ++q) {
        unsigned long long t = 0;
        for (int sl = 0; sl < kDiffSlots; ++sl) t += h[4 * sl + q];
        out[q] = (int64_t)t;
    }
    return AIY_OK;
}

int aiy_ws_screen_paths(aiy_ws* ws, int64_t out[2]) {
    if (!ws || !out) return fail(AIY_BAD_ARG, "NULL workspace/out");
    std::vector<unsigned long long> h(kHitcountLen, 0ull);
    if (ws->hitcount)
        AIY_HIP(hipMemcpy(h.data(), ws->hitcount, h.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
    for (int q = 0; q < 2; ++q) {
        unsigned long long t = 0;
        for (int sl = 0; sl < kDiffSlots; ++sl) t += h[kPathBase + 4 * sl + q];
        out[q] = (int64_t)t;
    }
    return AIY_OK;
}

int aiy_ws_trace(aiy_ws* ws, int64_t* out, int64_t cap, int64_t* n) {
    if (!ws || !out || !n) return fail(AIY_BAD_ARG, "NULL argument");
    *n = 0;
    if (!ws->trace) return AIY_OK;
    int64_t m = std::min(cap, ws_trace_units(ws));
    AIY_HIP(hipMemcpy(out, ws->trace, 16 * (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost));
    *n = m;
    return AIY_OK;
}

int aiy_ws_invalidate(aiy_ws* ws) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    ws->kf_ok = false;
    ws->dis_ok = false;
    return AIY_OK;
}

int aiy_ws_set_variant(aiy_ws* ws, int variant) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (variant < -1 || variant >= (1 << 30)) return fail(AIY_BAD_ARG, "variant in [-1, 2^30)");
    ws->variant = variant;
    return AIY_OK;
}

int aiy_ws_set_wide(aiy_ws* ws, int max_na, int splits, int waves, int states) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (max_na < -1 || splits < 0 || splits > kWideMaxSplits ||
        (waves != 0 && waves != 4 && waves != 8 && waves != 16) ||
        (states != 0 && states != 8 && states != 16 && states != 32 && states != 64))
        return fail(AIY_BAD_ARG, "max_na >= -1, splits in [0, %d], waves in {0, 4, 8, 16}, "
                    "states in {0, 8, 16, 32, 64}", kWideMaxSplits);
    ws->wide_max = max_na;
    ws->wide_S = splits;
    ws->wide_NW = waves;
    ws->wide_SB = states;
    return AIY_OK;
}

int aiy_ws_set_cu_exclusive(aiy_ws* ws, int on) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    ws->cu_exclusive = on != 0;
    return AIY_OK;
}

int aiy_ws_set_speculation(aiy_ws* ws, int max_batch) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (max_batch < 0 || max_batch > 256) return fail(AIY_BAD_ARG, "max_batch in [0, 256]");
    if (max_batch != ws->spec_max) ws->spec = SpecRings{};
    ws->spec_max = max_batch;
    return AIY_OK;
}

int aiy_ws_set_search(aiy_ws* ws, int coarse_stride, int k_chunk) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (coarse_stride < 0 || k_chunk < 64 || k_chunk % 64)
        return fail(AIY_BAD_ARG, "coarse_stride >= 0, k_chunk >= 64 and a multiple of 64");
    if (coarse_stride) ws->coarse = coarse_stride;
    if (k_chunk != ws->CK) {
        ws->CK = k_chunk;
        ws->partial.release();  // refilled (-1) at the next sweep
    }
    return AIY_OK;
}

int aiy_vfi_sweep_dev(aiy_ws* ws, const double* v_old, const double* a_grid, const double* s,
                      const double* P, double r, double w, double beta, double sigma,
                      const int32_t* hint, int mode, double* v_new, int32_t* idx,
                      double* policy_k, double* policy_c, double* diff, void* stream) {
    BellCall c{};
    c.v_old = v_old; c.a = a_grid; c.s = s; c.P = P; c.r = r; c.w = w; c.beta = beta;
    c.sigma = sigma; c.hint = hint; c.mode = mode; c.v_new = v_new; c.idx = idx;
    c.pk = policy_k; c.pc = policy_c; c.diff_out = diff;
    return bell_sweep_dev(ws, c, (hipStream_t)stream);
}

int aiy_vfi_sweeps_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                       const double* s, const double* P, double r, double w, double beta,
                       double sigma, const int32_t* hint, int64_t nsweeps, int mode, int32_t* idx,
                       double* policy_k, double* policy_c, double* diff, void* stream) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (nsweeps < 1) return fail(AIY_BAD_ARG, "nsweeps >= 1");
    if (!v_a || !v_b || v_a == v_b) return fail(AIY_BAD_ARG, "two distinct value buffers");
    if (!idx) return fail(AIY_BAD_ARG, "NULL idx (the next sweep's hint)");
    BellCall c{};
    c.a = a_grid; c.s = s; c.P = P; c.r = r; c.w = w; c.beta = beta; c.sigma = sigma;
    c.mode = mode; c.idx = idx; c.pk = policy_k; c.pc = policy_c;
    for (int64_t g = 0; g < nsweeps; ++g) {  // sweep g + 1 of the plain loop: ping-pong v_a / v_b
        c.v_old = (g & 1) ? v_b : v_a;
        c.v_new = (g & 1) ? v_a : v_b;
        c.hint = g ? idx : hint;
        c.diff_out = (g == nsweeps - 1) ? diff : nullptr;
        AIY_TRY(bell_sweep_dev(ws, c, (hipStream_t)stream));
    }
    return AIY_OK;
}

int aiy_vfi_solve_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                      const double* s, const double* P, double r, double w, double beta,
                      double sigma, double tol, int64_t max_iter, int mode, int32_t* idx,
                      double* policy_k, double* policy_c, int64_t* iters, int* out_new,
                      void* stream) {
    if (!iters || !out_new) return fail(AIY_BAD_ARG, "NULL iters/out_new");
    BellCall c{};
    c.a = a_grid; c.s = s; c.P = P; c.r = r; c.w = w; c.beta = beta; c.sigma = sigma;
    c.mode = mode; c.idx = idx; c.pk = policy_k; c.pc = policy_c;
    return bell_solve_dev(ws, c, v_a, v_b, tol, max_iter, iters, out_new, (hipStream_t)stream);
}

int aiy_vfi_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                            double* v_a, double* v_b, const double* a_grid, const double* s,
                            const double* P, double beta, double sigma, double tol,
                            int64_t max_iter, int use_hint, int32_t* idx, double* policy_k,
                            double* policy_c, int64_t* iters, int32_t* which, void* stream) {
    return bell_solve_batch_dev(ws, C, r, w, v_a, v_b, a_grid, s, P, beta, sigma, tol, max_iter,
                                use_hint, idx, policy_k, policy_c, iters, which,
                                (hipStream_t)stream);
}

int aiy_labor_vfi_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                                  double* v_a, double* v_b, const double* a_grid,
                                  const double* s, const double* P, const double* labor_choice,
                                  double beta, double sigma, double psi, double eta, double tol,
                                  int64_t max_iter, int use_hint, int32_t* lin, double* policy_k,
                                  double* policy_l, double* policy_c, int64_t* iters,
                                  int32_t* which, void* stream) {
    return bell_labor_solve_batch_dev(ws, C, r, w, v_a, v_b, a_grid, s, P, labor_choice, beta,
                                      sigma, psi, eta, tol, max_iter, use_hint, lin, policy_k,
                                      policy_l, policy_c, iters, which, (hipStream_t)stream);
}

int aiy_ws_set_labor_batch(aiy_ws* ws, int min_candidates) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (min_candidates < 0) return fail(AIY_BAD_ARG, "min_candidates >= 0 (0: the default)");
    ws->labor_batch_min = min_candidates;
    return AIY_OK;
}

int aiy_ws_labor_batch_counts(aiy_ws* ws, int64_t* batched_solves, int64_t* fallback_solves) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (batched_solves) *batched_solves = ws->labor_batch_solves;
    if (fallback_solves) *fallback_solves = ws->labor_batch_fallbacks;
    return AIY_OK;
}

int aiy_labor_vfi_sweep_dev(aiy_ws* ws, const double* v_old, const double* a_grid,
                            const double* s, const double* P, const double* labor_choice,
                            double r, double w, double beta, double sigma, double psi,
                            double eta, const int32_t* hint, double* v_new, int32_t* lin,
                            double* policy_k, double* policy_l, double* policy_c, double* diff,
                            void* stream) {
    BellCall c{};
    c.labor = true; c.Nl = ws ? ws->Nl : 0; c.L = labor_choice; c.psi = psi; c.eta = eta;
    c.v_old = v_old; c.a = a_grid; c.s = s; c.P = P; c.r = r; c.w = w; c.beta = beta;
    c.sigma = sigma; c.hint = hint; c.v_new = v_new; c.idx = lin; c.pk = policy_k;
    c.pl = policy_l; c.pc = policy_c; c.diff_out = diff;
    return bell_sweep_dev(ws, c, (hipStream_t)stream);
}

int aiy_labor_vfi_sweeps_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                             const double* s, const double* P, const double* labor_choice,
                             double r, double w, double beta, double sigma, double psi,
                             double eta, const int32_t* hint, int64_t nsweeps, int32_t* lin,
                             double* policy_k, double* policy_l, double* policy_c, double* diff,
                             void* stream) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (nsweeps < 1) return fail(AIY_BAD_ARG, "nsweeps >= 1");
    if (!v_a || !v_b || v_a == v_b) return fail(AIY_BAD_ARG, "two distinct value buffers");
    if (!lin) return fail(AIY_BAD_ARG, "NULL lin (the next sweep's hint)");
    BellCall c{};
    c.labor = true; c.Nl = ws->Nl; c.L = labor_choice; c.psi = psi; c.eta = eta;
    c.a = a_grid; c.s = s; c.P = P; c.r = r; c.w = w; c.beta = beta; c.sigma = sigma;
    c.idx = lin; c.pk = policy_k; c.pl = policy_l; c.pc = policy_c;
    for (int64_t g = 0; g < nsweeps; ++g) {  // sweep g + 1 of the loop: ping-pong v_a / v_b
        c.v_old = (g & 1) ? v_b : v_a;
        c.v_new = (g & 1) ? v_a : v_b;
        c.hint = g ? lin : hint;
        c.keep_incoming = (g == 0);
        c.diff_out = (g == nsweeps - 1) ? diff : nullptr;
        AIY_TRY(bell_sweep_dev(ws, c, (hipStream_t)stream));
    }
    return AIY_OK;
}

}  // extern "C"
