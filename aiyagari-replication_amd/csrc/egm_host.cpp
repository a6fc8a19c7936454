// A4/A5 entry points: device tier (aiy_egm_step_dev, aiy_egm_solve_dev and the batched
// multi-rate aiy_egm_solve_batch_dev) and MATLAB host tier (aiy_egm_*, aiy_labor_egm_*).
// policy arrays are Na x N column-major == [N][Na]: no transposes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "egm.hpp"
#include "host_ctx.hpp"
#include "spec_loop.hpp"
#include "ws.hpp"

namespace aiy {

// set by fail_nonmonotone: lets the batched solve's per-candidate fallback tell this failure
// (a candidate's status) from every other (the call's)
static thread_local bool t_nonmonotone = false;

static int fail_nonmonotone() {
    t_nonmonotone = true;
    return fail(AIY_BAD_ARG, "endogenous grid a_hat is not increasing: interp1 in the "
                             "reference would sort it or fail (Aiyagari_EGM.m:95)");
}

// the non-monotone flag of a step from host copies of its diff slots and flag word: bit 0 of
// the word (two-launch step) or bit 1 of a slot's second word (egm_fused_kernel)
static bool egm_nonmonotone(const unsigned long long* slots, unsigned flag_word) {
    if (flag_word & 1u) return true;
    for (int q = 0; q < kDiffSlots; ++q)
        if (slots[2 * q + 1] & 2ull) return true;
    return false;
}

static int ensure_egm(aiy_ws* ws) {
    const size_t n = (size_t)ws->N * ws->Na;
    bool fresh;
    AIY_TRY(ws->g0.ensure(n));
    AIY_TRY(ws->g1.ensure(n));
    AIY_TRY(ws->gi.ensure(16));
    AIY_TRY(ws_ensure_diff(ws));
    if (ws->tracing) {  // (instrumentation) one record per interp / chain wave: N·ntile
        AIY_TRY(ws_ensure_trace(ws, (int64_t)ws->N * ((ws->Na + 15) / 16), &fresh));
        if (fresh) AIY_HIP(hipMemset(ws->trace, 0, ws->trace.cap() * sizeof(long long)));
    }
    AIY_TRY(ws->egm_seg.ensure(n, &fresh));
    if (fresh) AIY_HIP(hipMemset(ws->egm_seg, 0xff, n * sizeof(int)));  // -1: no hint yet
    return AIY_OK;
}

static EgmArgs egm_args(aiy_ws* ws, const double* c, const double* a, const double* s,
                        const double* P, double r, double w, double beta, double sigma,
                        double amin, bool labor, double phi, double theta, double* cout,
                        double* pk, double* pl) {
    EgmArgs A{};
    A.N = (int)ws->N;
    A.Na = (int)ws->Na;
    A.labor = labor;
    A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
    A.r = r; A.w = w; A.beta = beta; A.sigma = sigma; A.amin = amin; A.phi = phi;
    A.theta = theta;
    A.c = c; A.a = a; A.s = s; A.P = P;
    A.ahat = ws->g0; A.cnext = ws->g1; A.cout = cout; A.pk = pk; A.pl = pl;
    A.diff = ws->diff;
    A.flags = ws->gi;
    A.trace = ws->tracing ? ws->trace : nullptr;  // (instrumentation; see ensure_egm)
    // interp1 segment hints (verified in the kernel; kEgmNoHints turns them off, A/B only)
    A.seg = egm_knob(ws, kEgmNoHints) ? nullptr : ws->egm_seg;
    // small grids: one launch per step (egm_fused_kernel) unless kEgmTwoLaunch; large grids:
    // the two-launch step (the solve loop chains it, egm_solve_spec).  (A one-pass scatter step
    // was measured slower — 35.6 vs 12.1 us at Na = 20,000, DESIGN.md §5 — and removed.)
    A.fused = !egm_knob(ws, kEgmTwoLaunch);
    return A;
}

int egm_step_dev(aiy_ws* ws, const double* c, const double* a, const double* s, const double* P,
                 double r, double w, double beta, double sigma, double amin, bool labor,
                 double phi, double theta, double* cout, double* pk, double* pl, double* diff_out,
                 hipStream_t st) {
    if (!ws || !c || !a || !s || !P || !cout || !pk) return fail(AIY_BAD_ARG, "NULL argument");
    if (labor && !(phi == phi && theta == theta)) return fail(AIY_NON_FINITE, "phi/theta");
    AIY_TRY(ensure_egm(ws));
    EgmArgs A = egm_args(ws, c, a, s, P, r, w, beta, sigma, amin, labor, phi, theta, cout, pk, pl);
    // the two-launch and small-grid steps clear ws->diff and the flag word themselves
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_egm_step(A, st));
    AIY_TRY(ws_timing_end(ws, st));
    if (diff_out) AIY_TRY(launch_reduce_slots(ws->diff, diff_out, st));
    return AIY_OK;
}

// dist of the last step + the non-monotone-grid flag (synchronises)
static int read_egm(aiy_ws* ws, hipStream_t st, double* d) {
    unsigned long long* h = ws->hdiff;
    AIY_HIP(hipMemcpyAsync(h, ws->diff, 2 * kDiffSlots * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st));
    AIY_HIP(hipMemcpyAsync(h + 2 * kDiffSlots, ws->gi, sizeof(int), hipMemcpyDeviceToHost, st));
    AIY_HIP(hipStreamSynchronize(st));
    *d = fold_slots_host(h);
    if (egm_nonmonotone(h, (unsigned)h[2 * kDiffSlots])) return fail_nonmonotone();
    return AIY_OK;
}

// The solve loop (Aiyagari_EGM.m:74-108, labour :67-105) with speculative batches, the loop of
// the VFI solve (spec_loop.hpp; bell_host.cpp, bell_solve_spec): steps are deterministic, so
// batches of m steps are enqueued between reads — step g reads ring slot (g−1) mod R and writes
// slot g mod R, its dist lands in slot set g mod R with its flag word (a chained step zeroes set
// (g+1) mod R for the next step; the other steps clear their own) — and each batch ends with one
// D2H copy of the slot sets and an event.  Two batches are in flight: the host reads batch
// k's dists while batch k+1 runs, so the device never idles at a read; with R = 2M + 1 slots
// the stopping step's policy_c survives the next batch's writes.  Its policy_k (and policy_l)
// were overwritten by later speculative steps, so the stopping step is re-run from its input
// (identical values).  Iteration count, dist and outputs equal the one-read-per-step loop's.
static int egm_solve_spec(aiy_ws* ws, const EgmArgs& A0, double* c0, double tol,
                          int64_t max_iter, double** cur_out, double* dist, int64_t* iters,
                          hipStream_t st) {
    const int M = ws->spec_max, R = 2 * M + 1;
    const size_t n = (size_t)ws->N * ws->Na, nb = n * sizeof(double);
    const int SW = kEgmSlotWords;  // per step: {max bits, any} slots, then the flag word
    const size_t SB = (size_t)R * SW * sizeof(unsigned long long);
    SlotRings& eg = ws->egm;
    AIY_TRY(eg.ensure(n, M, SW));
    auto slot = [&](int64_t g) { return eg.ring + (size_t)(g % R) * n; };
    auto sset = [&](int64_t g) { return eg.slots + (size_t)(g % R) * SW; };
    AIY_HIP(hipMemcpyAsync(slot(0), c0, nb, hipMemcpyDeviceToDevice, st));
    // chained steps (the default for Na > 1,024): the RHS of step 1 here, then one launch per
    // step — interp1 of step g on â/c̃ pair (g−1) & 1, the RHS of step g+1 into pair g & 1
    const bool chain = !(A0.fused && A0.Na <= kEgmFusedMaxNa) && !egm_knob(ws, kEgmNoChain);
    if (chain) {
        AIY_TRY(ws->egm_x2.ensure(n));
        AIY_TRY(ws->egm_y2.ensure(n));
    }
    double* xs[2] = {ws->g0, ws->egm_x2};
    double* ys[2] = {ws->g1, ws->egm_y2};
    auto step = [&](int64_t g) {
        EgmArgs A = A0;
        A.c = slot(g - 1);
        A.cout = slot(g);
        A.diff = sset(g);
        A.flags = (unsigned*)(sset(g) + 2 * kDiffSlots);
        A.diff_clear = nullptr;
        if (!chain) return launch_egm_step(A, st);
        A.ahat = xs[(g - 1) & 1];
        A.cnext = ys[(g - 1) & 1];
        A.ahat_next = xs[g & 1];
        A.cnext_next = ys[g & 1];
        A.diff_clear = sset(g + 1);
        AIY_TRY(ws_dispatch_arm(ws));  // (timing) the chained launch's own duration
        const int rc = launch_egm_chain(A, st);
        ws_dispatch_commit(ws);
        return rc;
    };
    if (chain) {  // step 1's RHS from slot 0; it clears step 1's slot set and flag word
        EgmArgs A = A0;
        A.c = slot(0);
        A.ahat = xs[0];
        A.cnext = ys[0];
        A.diff = sset(1);
        A.flags = (unsigned*)(sset(1) + 2 * kDiffSlots);
        AIY_TRY(launch_egm_rhs(A, st));
    }
    auto flush = [&](int hb) -> int {
        AIY_HIP(hipMemcpyAsync(eg.hslots + (size_t)hb * R * SW, eg.slots, SB,
                               hipMemcpyDeviceToHost, st));
        AIY_HIP(hipEventRecord(eg.ev[hb], st));
        return AIY_OK;
    };
    auto wait = [&](int hb) { return wait_event(eg.ev[hb]); };
    auto read = [&](int64_t g, int hb, double* d) -> int {
        const unsigned long long* h = eg.hslots + ((size_t)hb * R + (size_t)(g % R)) * SW;
        if (egm_nonmonotone(h, (unsigned)h[2 * kDiffSlots])) {
            AIY_HIP(hipStreamSynchronize(st));
            return fail_nonmonotone();
        }
        *d = fold_slots_host(h);
        return AIY_OK;
    };
    SpecResult S;
    AIY_TRY(spec_loop(M, max_iter, tol, &S, step, flush, wait, read,
                      [tol](double d) { return !(d > tol); }));  // Aiyagari_EGM.m:74 `while dist > tol`
    AIY_HIP(hipStreamSynchronize(st));  // (a speculative batch may still be running)
    const int64_t g = S.g, enq = S.enq;
    if (g > 0 && g != enq) {  // policy_k/l of the stopping step (its slots are not read
                              // again): the two-launch step from its input
        EgmArgs A = A0;
        A.c = slot(g - 1);
        A.cout = slot(g);
        A.diff = sset(g);
        A.flags = (unsigned*)(sset(g) + 2 * kDiffSlots);
        A.diff_clear = nullptr;
        AIY_TRY(launch_egm_step(A, st));
    }
    *cur_out = g > 0 ? slot(g) : slot(0);
    *dist = S.any ? S.d : 1.0;  // (no step: the loop's initial dist = 1)
    *iters = g;
    return AIY_OK;
}

static int egm_host(double* pc, const double* a, const double* s, const double* P, int64_t N,
                    int64_t Na, double r, double w, double beta, double sigma, double amin,
                    bool labor, double phi, double theta, bool solve, double tol,
                    int64_t max_iter, double* pcn_out, double* pk_out, double* pl_out,
                    double* dist, int64_t* iters) {
    if (!pc || !s || !P || !pk_out || !dist) return fail(AIY_BAD_ARG, "NULL argument");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    AIY_TRY(check_grid(a, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    double *da, *ds, *dP, *dc0, *dc1, *dpk, *dpl;
    AIY_TRY(stage_common(c, a, s, P, N, Na, &da, &ds, &dP));
    const size_t n = (size_t)N * Na;
    AIY_TRY(c->up("egm_c0", pc, n, &dc0));
    AIY_TRY(c->room("egm_c1", n, &dc1));
    AIY_TRY(c->room("pk", n, &dpk));
    AIY_TRY(c->room("pl", n, &dpl));
    double d = 1.0;
    int64_t it = 0;
    double* cur = dc0;
    double* nxt = dc1;
    if (!solve) {
        AIY_TRY(egm_step_dev(c->ws, cur, da, ds, dP, r, w, beta, sigma, amin, labor, phi, theta,
                             nxt, dpk, labor ? dpl : nullptr, nullptr, c->st));
        AIY_TRY(read_egm(c->ws, c->st, &d));
        cur = nxt;
        it = 1;
    } else if (c->ws->spec_max > 1 && max_iter > 0 && d > tol) {  // :74 tests dist = 1 first
        AIY_TRY(ensure_egm(c->ws));
        const EgmArgs A = egm_args(c->ws, cur, da, ds, dP, r, w, beta, sigma, amin, labor, phi,
                                   theta, nxt, dpk, labor ? dpl : nullptr);
        AIY_TRY(egm_solve_spec(c->ws, A, cur, tol, max_iter, &cur, &d, &it, c->st));
    } else {
        while (d > tol && it < max_iter) {  // Aiyagari_EGM.m:74
            ++it;
            AIY_TRY(egm_step_dev(c->ws, cur, da, ds, dP, r, w, beta, sigma, amin, labor, phi,
                                 theta, nxt, dpk, labor ? dpl : nullptr, nullptr, c->st));
            AIY_TRY(read_egm(c->ws, c->st, &d));
            std::swap(cur, nxt);  // :107 policy_c = policy_c_next
        }
    }
    double* dst = solve ? pc : pcn_out;
    if (dst) AIY_TRY(c->down(dst, cur, n));
    AIY_TRY(c->down(pk_out, dpk, n));
    if (labor && pl_out) AIY_TRY(c->down(pl_out, dpl, n));
    AIY_TRY(c->sync());
    *dist = d;
    if (iters) *iters = it;
    return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_egm_step(const double* policy_c, const double* a_grid, const double* s,
                 const double* P, int64_t N, int64_t Na, double r, double w, double beta,
                 double sigma, double amin, double* policy_c_next, double* policy_k,
                 double* dist) {
    if (!policy_c_next) return fail(AIY_BAD_ARG, "NULL policy_c_next");
    return egm_host(const_cast<double*>(policy_c), a_grid, s, P, N, Na, r, w, beta, sigma, amin,
                    false, 1, 1, false, 0, 1, policy_c_next, policy_k, nullptr, dist, nullptr);
}

int aiy_egm_solve(double* policy_c, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double amin, double tol, int64_t max_iter, double* policy_k, double* dist,
                  int64_t* iters) {
    return egm_host(policy_c, a_grid, s, P, N, Na, r, w, beta, sigma, amin, false, 1, 1, true,
                    tol, max_iter, nullptr, policy_k, nullptr, dist, iters);
}

int aiy_labor_egm_step(const double* policy_c, const double* a_grid, const double* s,
                       const double* P, int64_t N, int64_t Na, double r, double w, double beta,
                       double sigma, double phi, double theta, double amin,
                       double* policy_c_next, double* policy_k, double* policy_l,
                       double* dist) {
    if (!policy_c_next || !policy_l) return fail(AIY_BAD_ARG, "NULL output");
    return egm_host(const_cast<double*>(policy_c), a_grid, s, P, N, Na, r, w, beta, sigma, amin,
                    true, phi, theta, false, 0, 1, policy_c_next, policy_k, policy_l, dist,
                    nullptr);
}

int aiy_labor_egm_solve(double* policy_c, const double* a_grid, const double* s,
                        const double* P, int64_t N, int64_t Na, double r, double w,
                        double beta, double sigma, double phi, double theta, double amin,
                        double tol, int64_t max_iter, double* policy_k, double* policy_l,
                        double* dist, int64_t* iters) {
    if (!policy_l) return fail(AIY_BAD_ARG, "NULL policy_l");
    return egm_host(policy_c, a_grid, s, P, N, Na, r, w, beta, sigma, amin, true, phi, theta,
                    true, tol, max_iter, nullptr, policy_k, policy_l, dist, iters);
}

int aiy_egm_solve_dev(aiy_ws* ws, double* policy_c, const double* a_grid, const double* s,
                      const double* P, double r, double w, double beta, double sigma,
                      double amin, int labor, double phi, double theta, double tol,
                      int64_t max_iter, double* policy_k, double* policy_l, int64_t* iters,
                      double* dist, void* stream) {
    if (!ws || !policy_c || !a_grid || !s || !P || !policy_k || !iters || !dist)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (labor && !(phi == phi && theta == theta)) return fail(AIY_NON_FINITE, "phi/theta");
    if (max_iter < 0) return fail(AIY_BAD_ARG, "max_iter must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    AIY_TRY(ensure_egm(ws));
    const size_t nb = sizeof(double) * ws->N * ws->Na;
    double d = 1.0;
    int64_t it = 0;
    if (max_iter > 0 && d > tol) {  // Aiyagari_EGM.m:74 tests dist = 1 first
        if (ws->spec_max > 1) {
            const EgmArgs A = egm_args(ws, policy_c, a_grid, s, P, r, w, beta, sigma, amin,
                                       labor != 0, phi, theta, nullptr, policy_k,
                                       labor ? policy_l : nullptr);
            double* cur = nullptr;
            AIY_TRY(egm_solve_spec(ws, A, policy_c, tol, max_iter, &cur, &d, &it, st));
            AIY_HIP(hipMemcpyAsync(policy_c, cur, nb, hipMemcpyDeviceToDevice, st));
        } else {
            AIY_TRY(ws->g2.ensure((size_t)ws->N * ws->Na));
            double* nxt = ws->g2;
            while (d > tol && it < max_iter) {  // :74 (one read per step)
                ++it;
                AIY_TRY(egm_step_dev(ws, policy_c, a_grid, s, P, r, w, beta, sigma, amin,
                                     labor != 0, phi, theta, nxt, policy_k,
                                     labor ? policy_l : nullptr, nullptr, st));
                AIY_TRY(read_egm(ws, st, &d));
                AIY_HIP(hipMemcpyAsync(policy_c, nxt, nb, hipMemcpyDeviceToDevice, st));
            }
        }
    }
    AIY_HIP(hipStreamSynchronize(st));
    *iters = it;
    *dist = d;
    return AIY_OK;
}

int aiy_egm_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                            double* policy_c, const double* a_grid, const double* s,
                            const double* P, double beta, double sigma, double amin, int labor,
                            double phi, double theta, double tol, int64_t max_iter,
                            double* policy_k, double* policy_l, int64_t* iters, double* dist,
                            int32_t* status, void* stream) {
    if (!ws || !r || !w || !policy_c || !a_grid || !s || !P || !policy_k || !iters || !dist ||
        !status || (labor && !policy_l))
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (ws->N > 16) return fail(AIY_BAD_SHAPE, "EGM kernels support N <= 16 productivity states");
    if (ws->Na < 2) return fail(AIY_BAD_SHAPE, "need Na >= 2");
    if (labor && !(phi == phi && theta == theta)) return fail(AIY_NON_FINITE, "phi/theta");
    if (max_iter < 0) return fail(AIY_BAD_ARG, "max_iter must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)ws->N * ws->Na;
    if (!(max_iter > 0 && 1.0 > tol)) {  // Aiyagari_EGM.m:74 tests dist = 1 first: no step
        for (int64_t c = 0; c < C; ++c) {
            iters[c] = 0;
            dist[c] = 1.0;
            status[c] = 0;
        }
        AIY_HIP(hipStreamSynchronize(st));
        return AIY_OK;
    }
    const int64_t min_c = ws->egm_batch_min < 0 ? egm_batch_min_c(ws->N, ws->Na) : ws->egm_batch_min;
    if (min_c > 0 && C >= min_c && egm_batch_fits(ws->N, ws->Na, labor != 0)) {
        EgmBatchBlocks& bb = ws->egm_batch;
        AIY_TRY(bb.ensure((size_t)C));
        std::memcpy(bb.hrw.get(), r, sizeof(double) * C);
        std::memcpy(bb.hrw.get() + C, w, sizeof(double) * C);
        AIY_HIP(hipMemcpyAsync(bb.rw, bb.hrw, sizeof(double) * 2 * C, hipMemcpyHostToDevice, st));
        EgmBatchArgs A{};
        A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C;
        A.labor = labor != 0;
        A.ns = is_int_ge(sigma, 1.0) ? (int)sigma : 0;
        A.beta = beta; A.sigma = sigma; A.amin = amin; A.phi = phi; A.theta = theta; A.tol = tol;
        A.max_iter = max_iter;
        A.r = bb.rw; A.w = bb.rw + C;
        A.a = a_grid; A.s = s; A.P = P;
        A.c = policy_c; A.pk = policy_k; A.pl = labor ? policy_l : nullptr;
        A.iters = bb.iters; A.dist = bb.dist; A.status = bb.status;
        AIY_TRY(ws_timing_begin(ws, st));
        AIY_TRY(launch_egm_solve_batch(A, st));
        AIY_TRY(ws_timing_end(ws, st));
        ++ws->egm_batch_launches;
        AIY_HIP(hipMemcpyAsync(bb.hiters, bb.iters, sizeof(long long) * C, hipMemcpyDeviceToHost, st));
        AIY_HIP(hipMemcpyAsync(bb.hdist, bb.dist, sizeof(double) * C, hipMemcpyDeviceToHost, st));
        AIY_HIP(hipMemcpyAsync(bb.hstatus, bb.status, sizeof(int) * C, hipMemcpyDeviceToHost, st));
        AIY_HIP(hipStreamSynchronize(st));  // the call's one synchronisation
        for (int64_t c = 0; c < C; ++c) {
            iters[c] = (int64_t)bb.hiters[c];
            dist[c] = bb.hdist[c];
            status[c] = bb.hstatus[c];
        }
        return AIY_OK;
    }
    // shapes whose arrays do not fit one CU's LDS, and fewer candidates than the threshold: the
    // existing solve, one candidate after another; its non-monotone error is that candidate's
    // status, not the call's
    for (int64_t c = 0; c < C; ++c) {
        t_nonmonotone = false;
        const int rc = aiy_egm_solve_dev(ws, policy_c + c * n, a_grid, s, P, r[c], w[c], beta, sigma,
                                         amin, labor, phi, theta, tol, max_iter, policy_k + c * n,
                                         labor ? policy_l + c * n : nullptr, iters + c, dist + c,
                                         stream);
        ++ws->egm_batch_fallbacks;
        status[c] = 0;
        if (rc != AIY_OK) {
            if (!t_nonmonotone) return rc;
            status[c] = 1;
            iters[c] = 0;
            dist[c] = NAN;
        }
    }
    return AIY_OK;
}

int aiy_ws_set_egm_batch(aiy_ws* ws, int min_candidates) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (min_candidates < -1) return fail(AIY_BAD_ARG, "min_candidates must be >= -1");
    ws->egm_batch_min = min_candidates;
    return AIY_OK;
}

int aiy_ws_egm_batch_counts(aiy_ws* ws, int64_t* launches, int64_t* fallback_solves) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (launches) *launches = ws->egm_batch_launches;
    if (fallback_solves) *fallback_solves = ws->egm_batch_fallbacks;
    return AIY_OK;
}

int aiy_egm_step_dev(aiy_ws* ws, const double* policy_c, const double* a_grid,
                     const double* s, const double* P, double r, double w, double beta,
                     double sigma, double amin, int labor, double phi, double theta,
                     double* policy_c_next, double* policy_k, double* policy_l, double* diff,
                     void* stream) {
    return egm_step_dev(ws, policy_c, a_grid, s, P, r, w, beta, sigma, amin, labor != 0, phi,
                        theta, policy_c_next, policy_k, policy_l, diff, (hipStream_t)stream);
}

}  // extern "C"
