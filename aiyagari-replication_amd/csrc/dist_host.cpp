// A10 entry points: aiy_dist_update_dev (one histogram push on device),
// aiy_dist_stationary_dev (iterate to the fixed point on device), aiy_dist_stationary
// (MATLAB layouts, K = Σ λ·a) and their forms for C candidate policies at once
// (aiy_dist_stationary_batch_dev, aiy_dist_stationary_batch).
//
// The policy is fixed across the fixed-point iteration, so its plan (keys, lottery weights,
// run offsets, the monotonicity flag) is built ONCE per call and read back once; every push is
// then one launch (dist_push_kernel).  The iteration runs in speculative batches as the VFI
// and EGM solves do (spec_loop.hpp): m pushes are enqueued per batch — push g reads ring slot
// (g−1) mod R and writes slot g mod R, its max|Δλ| lands in its own slot set — and the host reads
// one batch's slot sets while the next batch runs, to find the first push with max|Δλ| < tol.
// Pushes are deterministic, so the iteration count, the returned λ and dist are exactly the
// one-read-per-push loop's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "dist.hpp"
#include "host_ctx.hpp"
#include "spec_loop.hpp"
#include "ws.hpp"

namespace aiy {

constexpr int kDistSpecMax = 32;  // pushes per batch (two batches in flight)

static int ensure_dist(aiy_ws* ws) {
    const size_t n = (size_t)ws->N * ws->Na;
    AIY_TRY(ws->d_key.ensure(n));
    AIY_TRY(ws->d_off.ensure(n + ws->N));
    AIY_TRY(ws->d_wr.ensure(n));
    AIY_TRY(ws->d_mass.ensure(n));
    AIY_TRY(ws->d_part.ensure(260));
    AIY_TRY(ws->gi.ensure(16));
    return ws_ensure_diff(ws);
}

// the policy's plan; *fallback = the policy is not monotone (ordered-scan gather).
// Synchronises once to read the flags.
static int dist_plan(aiy_ws* ws, const int* idx, const double* kp, const double* a,
                     const double* P, DistArgs* A, bool* fallback, hipStream_t st) {
    if (!ws || !a || !P || (!idx && !kp))
        return fail(AIY_BAD_ARG, "NULL argument (need policy_idx or policy_k)");
    AIY_TRY(ensure_dist(ws));
    *A = DistArgs{};
    A->N = (int)ws->N; A->Na = (int)ws->Na; A->lottery = (idx == nullptr);
    A->idx = idx; A->kp = kp; A->a = a; A->P = P;
    A->key = ws->d_key; A->off = ws->d_off; A->wr = ws->d_wr; A->mass = ws->d_mass;
    A->diff = ws->diff; A->flags = ws->gi;
    A->trace = nullptr;
    if (ws->tracing) {  // (instrumentation) one record per push wave: ceil(Na/64)·N <= cap
        const int64_t cap = (int64_t)ws->N * ((ws->Na + 15) / 16);
        AIY_TRY(ws_ensure_trace(ws, cap));
        AIY_HIP(hipMemsetAsync(ws->trace, 0, 16 * (size_t)cap * sizeof(long long), st));
        A->trace = ws->trace;
    }
    AIY_HIP(hipMemsetAsync(ws->gi, 0, sizeof(int), st));
    AIY_TRY(launch_dist_prepare(*A, st));
    AIY_HIP(hipMemcpyAsync(&ws->hdiff[2 * kDiffSlots], ws->gi, sizeof(int), hipMemcpyDeviceToHost, st));
    AIY_HIP(hipStreamSynchronize(st));
    const unsigned flags = (unsigned)ws->hdiff[2 * kDiffSlots];
    if (flags & 2u) return fail(AIY_BAD_ARG, "policy index outside [1, Na]");
    *fallback = (flags & 1u) != 0;
    return AIY_OK;
}

// one push λ → λ'; *d_host = max|λ'−λ| (synchronising) when d_host != nullptr
int dist_update_dev(aiy_ws* ws, const double* lam, const int* idx, const double* kp,
                    const double* a, const double* P, double* out, double* diff_dev,
                    double* d_host, hipStream_t st) {
    if (!lam || !out) return fail(AIY_BAD_ARG, "NULL argument");
    DistArgs A;
    bool fb = false;
    AIY_TRY(dist_plan(ws, idx, kp, a, P, &A, &fb, st));
    A.lam = lam;
    A.out = out;
    AIY_HIP(hipMemsetAsync(ws->diff, 0, 2 * kDiffSlots * sizeof(unsigned long long), st));
    AIY_TRY(ws_timing_begin(ws, st));
    AIY_TRY(launch_dist_push(A, fb, st));
    AIY_TRY(ws_timing_end(ws, st));
    if (diff_dev) AIY_TRY(launch_reduce_slots(ws->diff, diff_dev, st));
    if (d_host) {
        AIY_HIP(hipMemcpyAsync(ws->hdiff, ws->diff, 2 * kDiffSlots * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, st));
        AIY_HIP(hipStreamSynchronize(st));
        *d_host = fold_slots_host(ws->hdiff);
    }
    return AIY_OK;
}

// the fixed-point loop of aiy_dist_stationary on device:  for it = 1..max_iter: push; stop
// when max|Δλ| < tol.  lam_out receives the last push; k_dev (nullable) = Σ λ·a.  Batches of
// pushes with one D2H copy of their diff slots and an event each; two batches in flight (the
// host reads batch k while batch k+1 runs), a ring of 2M + 1 λ buffers so that the stopping
// push's λ survives the next batch.
int dist_stationary_dev(aiy_ws* ws, const double* lam0, const int* idx, const double* kp,
                        const double* a, const double* P, double tol, int64_t max_iter,
                        double* lam_out, double* k_dev, int64_t* iters, double* dist,
                        hipStream_t st) {
    if (!lam0 || !lam_out || !iters || !dist) return fail(AIY_BAD_ARG, "NULL argument");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    DistArgs A0;
    bool fb = false;
    AIY_TRY(dist_plan(ws, idx, kp, a, P, &A0, &fb, st));
    const bool two_launch = fb || ws->N > kDistPushMaxN;  // (no diff_clear in those kernels)
    const int M = kDistSpecMax, R = 2 * M + 1;
    const size_t n = (size_t)ws->N * ws->Na, nb = n * sizeof(double);
    const int SW = 2 * kDiffSlots;
    const size_t SB = (size_t)R * SW * sizeof(unsigned long long);
    SlotRings& dr = ws->dist;
    AIY_TRY(dr.ensure(n, M, SW));
    auto slot = [&](int64_t g) { return dr.ring + (size_t)(g % R) * n; };
    auto sset = [&](int64_t g) { return dr.slots + (size_t)(g % R) * SW; };
    AIY_HIP(hipMemcpyAsync(slot(0), lam0, nb, hipMemcpyDeviceToDevice, st));
    AIY_HIP(hipMemsetAsync(sset(1), 0, SW * sizeof(unsigned long long), st));
    auto push = [&](int64_t g) -> int {
        DistArgs A = A0;
        A.lam = slot(g - 1);
        A.out = slot(g);
        A.diff = sset(g);
        // push g's set was zeroed by push g−1 (one-launch push) or is zeroed here
        if (two_launch) AIY_HIP(hipMemsetAsync(sset(g), 0, SW * sizeof(unsigned long long), st));
        else A.diff_clear = sset(g + 1);
        AIY_TRY(ws_dispatch_arm(ws));  // the push's own duration (one-launch push)
        const int rc = launch_dist_push(A, fb, st);
        ws_dispatch_commit(ws);
        return rc;
    };
    auto flush = [&](int hb) -> int {
        AIY_HIP(hipMemcpyAsync(dr.hslots + (size_t)hb * R * SW, dr.slots, SB,
                               hipMemcpyDeviceToHost, st));
        AIY_HIP(hipEventRecord(dr.ev[hb], st));
        return AIY_OK;
    };
    auto wait = [&](int hb) { return wait_event(dr.ev[hb]); };
    auto read = [&](int64_t g, int hb, double* d) -> int {
        *d = fold_slots_host(dr.hslots + ((size_t)hb * R + (size_t)(g % R)) * SW);
        return AIY_OK;
    };
    SpecResult S;
    AIY_TRY(spec_loop(M, max_iter, tol, &S, push, flush, wait, read,
                      [tol](double d) { return d < tol; }));
    const int64_t g = S.g;
    AIY_HIP(hipMemcpyAsync(lam_out, slot(g), nb, hipMemcpyDeviceToDevice, st));
    if (k_dev)
        AIY_TRY(launch_dist_capital(lam_out, a, (int)ws->N, (int)ws->Na, ws->d_part, k_dev, st));
    AIY_HIP(hipStreamSynchronize(st));  // (a speculative batch may still be running)
    *iters = g;
    *dist = S.d;
    return AIY_OK;
}

// The fixed points of C candidates (aiy_dist_stationary_batch_dev).  Batched path: one prepare
// launch pair builds all plans, the C flag words are read once (an out-of-range index fails the
// call before any solve), one launch solves every monotone candidate — a workgroup each, the
// loop in LDS — followed by the batched K, and one synchronisation reads iters and dist.
// Non-monotone candidates, and all of them when the shape does not fit or C is below the
// workspace's threshold, run dist_stationary_dev one after another: the same additions.
int dist_stationary_batch_dev(aiy_ws* ws, int64_t C, const double* lam0, const int* idx,
                              const double* kp, const double* a, const double* P, double tol,
                              int64_t max_iter, double* lam_out, double* k_dev, int64_t* iters,
                              double* dist, hipStream_t st) {
    if (!ws || !lam0 || !lam_out || !iters || !dist || !a || !P || (!idx && !kp))
        return fail(AIY_BAD_ARG, "NULL argument (need policy_idx or policy_k)");
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    const bool lottery = idx == nullptr;
    const size_t n = (size_t)ws->N * ws->Na, nw = n + (size_t)ws->N;
    const int64_t min_c = ws->dist_batch_min < 0 ? kDistBatchMinC : ws->dist_batch_min;
    const bool batched = min_c > 0 && C >= min_c && C <= 65535 &&
                         dist_batch_fits(ws->N, ws->Na, lottery);
    std::vector<char> separate((size_t)C, 1);  // candidates left to the per-candidate path
    if (batched) {
        DistBatchBlocks& bb = ws->dist_batch;
        AIY_TRY(bb.ensure((size_t)C, n, nw));
        DistBatchArgs A{};
        A.N = (int)ws->N; A.Na = (int)ws->Na; A.C = (int)C;
        A.lottery = lottery; A.tol = tol; A.max_iter = max_iter;
        A.idx = idx; A.kp = kp; A.a = a; A.P = P; A.lam = lam0; A.out = lam_out;
        A.key = bb.key; A.off = bb.off; A.wr = bb.wr; A.flags = bb.flags;
        A.iters = bb.iters; A.dist = bb.dist; A.part = bb.part; A.k = k_dev;
        AIY_HIP(hipMemsetAsync(bb.flags, 0, sizeof(unsigned) * C, st));
        AIY_TRY(launch_dist_batch_prepare(A, st));
        AIY_HIP(hipMemcpyAsync(bb.hflags, bb.flags, sizeof(unsigned) * C, hipMemcpyDeviceToHost, st));
        AIY_HIP(hipStreamSynchronize(st));
        int64_t nb = 0;
        for (int64_t c = 0; c < C; ++c) {
            if (bb.hflags[c] & 2u)
                return fail(AIY_BAD_ARG, "candidate %lld: policy index outside [1, Na]",
                            (long long)c + 1);
            separate[c] = bb.hflags[c] != 0u;
            nb += !separate[c];
        }
        if (nb > 0) {
            AIY_TRY(ws_timing_begin(ws, st));
            AIY_TRY(launch_dist_solve_batch(A, st));
            AIY_TRY(ws_timing_end(ws, st));
            ++ws->dist_batch_launches;
            AIY_HIP(hipMemcpyAsync(bb.hiters, bb.iters, sizeof(long long) * C, hipMemcpyDeviceToHost, st));
            AIY_HIP(hipMemcpyAsync(bb.hdist, bb.dist, sizeof(double) * C, hipMemcpyDeviceToHost, st));
            AIY_HIP(hipStreamSynchronize(st));  // the batched path's one synchronisation
            for (int64_t c = 0; c < C; ++c)
                if (!separate[c]) {
                    iters[c] = (int64_t)bb.hiters[c];
                    dist[c] = bb.hdist[c];
                }
        }
    } else if (idx) {
        // every candidate's indices are checked before the first solve, as on the batched path
        for (int64_t c = 0; c < C; ++c) {
            DistArgs A;
            bool fb = false;
            const int rc = dist_plan(ws, idx + c * n, nullptr, a, P, &A, &fb, st);
            if (rc == AIY_BAD_ARG)
                return fail(AIY_BAD_ARG, "candidate %lld: policy index outside [1, Na]",
                            (long long)c + 1);
            AIY_TRY(rc);
        }
    }
    for (int64_t c = 0; c < C; ++c) {
        if (!separate[c]) continue;
        AIY_TRY(dist_stationary_dev(ws, lam0 + c * n, idx ? idx + c * n : nullptr,
                                    kp && !idx ? kp + c * n : nullptr, a, P, tol, max_iter,
                                    lam_out + c * n, k_dev ? k_dev + c : nullptr, iters + c,
                                    dist + c, st));
        ++ws->dist_batch_fallbacks;
    }
    return AIY_OK;
}

// The host entries' staging and read-back, for C policies (aiy_dist_stationary: C = 1); each entry
// runs its own device tier in between.  Layouts: vfi_layout → N x Na column-major; else Na x N
// column-major (== [N][Na]).
struct DistStaged {
    double *a, *P, *l0, *l1, *kp = nullptr, *K;
    int* idx = nullptr;
};

static int dist_stage(HostCtx* c, int64_t C, const int32_t* policy_idx, const double* policy_k,
                      int vfi_layout, const double* a_grid, const double* P, int64_t N, int64_t Na,
                      const double* lambda, DistStaged* D) {
    const size_t n = (size_t)N * Na * C;
    std::vector<double> s1(N, 1.0);  // (only a and P are used here)
    double* ds;
    AIY_TRY(stage_common(c, a_grid, s1.data(), P, N, Na, &D->a, &ds, &D->P));
    auto rows_up = [&](const char* name, const double* src, double** dev) {
        return vfi_layout ? c->up_rows(name, src, N, Na, C, dev) : c->up(name, src, n, dev);
    };
    if (policy_idx)
        AIY_TRY(c->up_own("dist_idx", idx_rows0(policy_idx, vfi_layout, N, Na, C), &D->idx));
    else
        AIY_TRY(rows_up("dist_kp", policy_k, &D->kp));
    AIY_TRY(rows_up("dist_l0", lambda, &D->l0));
    AIY_TRY(c->room("dist_l1", n, &D->l1));
    return c->room("dist_K", std::max<size_t>((size_t)C, 2), &D->K);
}

// λ and K of the C candidates back (synchronises)
static int dist_back(HostCtx* c, const DistStaged& D, int64_t C, int vfi_layout, int64_t N,
                     int64_t Na, double* lambda, double* k_supply) {
    AIY_TRY(c->down(k_supply, D.K, (size_t)C));
    if (vfi_layout) return c->down_rows(lambda, D.l1, N, Na, C);
    AIY_TRY(c->down(lambda, D.l1, (size_t)N * Na * C));
    return c->sync();
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_dist_update_dev(aiy_ws* ws, const double* lambda, const int32_t* policy_idx,
                        const double* policy_k, const double* a_grid, const double* P,
                        double* lambda_out, double* diff, void* stream) {
    return dist_update_dev(ws, lambda, policy_idx, policy_k, a_grid, P, lambda_out, diff,
                           nullptr, (hipStream_t)stream);
}

int aiy_dist_stationary_dev(aiy_ws* ws, const double* lambda, const int32_t* policy_idx,
                            const double* policy_k, const double* a_grid, const double* P,
                            double tol, int64_t max_iter, double* lambda_out,
                            double* k_supply, int64_t* iters, double* dist, void* stream) {
    return dist_stationary_dev(ws, lambda, policy_idx, policy_k, a_grid, P, tol, max_iter,
                               lambda_out, k_supply, iters, dist, (hipStream_t)stream);
}

int aiy_dist_stationary(const int32_t* policy_idx, const double* policy_k, int vfi_layout,
                        const double* a_grid, const double* P, int64_t N, int64_t Na,
                        double tol, int64_t max_iter, double* lambda, double* k_supply,
                        int64_t* iters, double* dist) {
    if ((!policy_idx && !policy_k) || !P || !lambda || !k_supply || !iters || !dist)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    // the lottery divides by a(k+1) - a(k): repeated nodes are rejected (interp1 would error)
    AIY_TRY(policy_k ? check_grid_strict(a_grid, Na) : check_grid(a_grid, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    DistStaged D;
    AIY_TRY(dist_stage(c, 1, policy_idx, policy_k, vfi_layout, a_grid, P, N, Na, lambda, &D));
    double d = NAN;
    int64_t it = 0;
    AIY_TRY(dist_stationary_dev(c->ws, D.l0, D.idx, D.kp, D.a, D.P, tol, max_iter, D.l1, D.K, &it,
                                &d, c->st));
    AIY_TRY(dist_back(c, D, 1, vfi_layout, N, Na, lambda, k_supply));
    *iters = it;
    *dist = d;
    return AIY_OK;
}

int aiy_dist_stationary_batch_dev(aiy_ws* ws, int64_t C, const double* lambda,
                                  const int32_t* policy_idx, const double* policy_k,
                                  const double* a_grid, const double* P, double tol,
                                  int64_t max_iter, double* lambda_out, double* k_supply,
                                  int64_t* iters, double* dist, void* stream) {
    return dist_stationary_batch_dev(ws, C, lambda, policy_idx, policy_k, a_grid, P, tol, max_iter,
                                     lambda_out, k_supply, iters, dist, (hipStream_t)stream);
}

int aiy_ws_set_dist_batch(aiy_ws* ws, int min_candidates) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (min_candidates < -1) return fail(AIY_BAD_ARG, "min_candidates must be >= -1");
    ws->dist_batch_min = min_candidates;
    return AIY_OK;
}

int aiy_ws_dist_batch_counts(aiy_ws* ws, int64_t* launches, int64_t* fallback_solves) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (launches) *launches = ws->dist_batch_launches;
    if (fallback_solves) *fallback_solves = ws->dist_batch_fallbacks;
    return AIY_OK;
}

int aiy_dist_stationary_batch(int64_t C, const int32_t* policy_idx, const double* policy_k,
                              int vfi_layout, const double* a_grid, const double* P, int64_t N,
                              int64_t Na, double tol, int64_t max_iter, double* lambda,
                              double* k_supply, int64_t* iters, double* dist) {
    if ((!policy_idx && !policy_k) || !P || !lambda || !k_supply || !iters || !dist)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (N < 1 || Na < 2) return fail(AIY_BAD_SHAPE, "need N >= 1 and Na >= 2");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    AIY_TRY(!policy_idx ? check_grid_strict(a_grid, Na) : check_grid(a_grid, Na));
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(N, Na, 1, &c));
    DistStaged D;
    AIY_TRY(dist_stage(c, C, policy_idx, policy_k, vfi_layout, a_grid, P, N, Na, lambda, &D));
    AIY_TRY(dist_stationary_batch_dev(c->ws, C, D.l0, D.idx, D.kp, D.a, D.P, tol, max_iter, D.l1,
                                      D.K, iters, dist, c->st));
    return dist_back(c, D, C, vfi_layout, N, Na, lambda, k_supply);
}

}  // extern "C"
