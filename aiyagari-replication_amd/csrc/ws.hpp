// Workspace (aiy_ws): per-shape device scratch owned by the library, reused across calls.
// Every allocation is a DevBuf / PinnedBuf / Events member (devbuf.hpp), sized where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include "aiy_common.hpp"
#include "bellman.hpp"
#include "devbuf.hpp"

namespace aiy {
using u64 = unsigned long long;
// speculative VFI solve (bell_solve_spec): ring of 2m + 1 value buffers, 2m policy sets and one
// folded-diff pair per sweep of a batch, for n states and m = spec_max
struct SpecRings {
    size_t n = 0;  // states per buffer the rings were sized for (0 = not allocated)
    int m = 0;     // spec_max the rings were sized for
    DevBuf<double> v;
    DevBuf<int> idx;
    DevBuf<double> pol;    // [2m][3][n] (k, c, l)
    DevBuf<u64> diff;      // device [2 * 2m]: a pair per sweep
    PinnedBuf<u64> hdiff;  // two copies (batches in flight)
    Events ev;             // [2] end of each in-flight batch's copy
};
// speculative EGM solve (ring of policy_c, slot sets of 2*kDiffSlots + 2 words: diff slots + the
// flag word) and speculative histogram iteration (ring of λ, slot sets of 2*kDiffSlots words):
// 2m + 1 buffers of n doubles, a slot set per step
struct SlotRings {
    size_t n = 0;
    int m = 0;
    DevBuf<double> ring;
    DevBuf<u64> slots;      // device [2m + 1][slot set]
    PinnedBuf<u64> hslots;  // two copies (batches in flight)
    Events ev;              // [2] end of each in-flight batch's slot copy
    // sized for (n_, m_) with W words per slot set; another (n, m) drops the old rings first
    int ensure(size_t n_, int m_, size_t W) {
        if (n == n_ && m == m_) return AIY_OK;
        *this = SlotRings{};
        const size_t R = 2 * (size_t)m_ + 1;
        AIY_TRY(ring.ensure(R * n_));
        AIY_TRY(slots.ensure(R * W));
        AIY_TRY(hslots.ensure(2 * R * W));
        AIY_TRY(ev.create(2, hipEventDisableTiming));
        n = n_;
        m = m_;
        return AIY_OK;
    }
};
// C candidate rates solved in lockstep (bell_lockstep): the candidates' prices, the sweep each
// stopped at (0 = running) and the host copies the driver reads
struct LockstepBlocks {
    DevBuf<int> stop;       // device [C]
    DevBuf<double> rw;      // device [2][C]: r then w
    PinnedBuf<int> hstop;   // [C]
    PinnedBuf<u64> hslots;  // [C][2*kDiffSlots]: slot sets of the candidates still running
    int ensure(size_t C) {
        AIY_TRY(stop.ensure(C));
        AIY_TRY(rw.ensure(2 * C));
        AIY_TRY(hstop.ensure(C));
        return hslots.ensure(C * 2 * kDiffSlots);
    }
};
// batched candidate rates (config 4, aiy_vfi_solve_batch_dev): per-candidate blocks of the
// tree-screen scratch, sized for C candidates
struct BatchBlocks {
    int64_t C = 0;
    DevBuf<double> EV, Dt, Dm8, Dm512, best0;
    DevBuf<int> idx0, mom, kf;
    DevBuf<u64> slots;      // device [C][2][2*kDiffSlots]
    LockstepBlocks ls;
};
// batched labour solve on the small-grid sweep (aiy_labor_vfi_solve_batch_dev): per-candidate
// feasible prefixes and three slot sets each (wide_batch.hpp), sized for C candidates
struct LaborBatchBlocks {
    int64_t C = 0;
    DevBuf<int> kf;         // device [C][Nl][N][Na]
    DevBuf<u64> slots;      // device [C][3][2*kDiffSlots]
    LockstepBlocks ls;
};
// transition passes (aiy_egm_backward_batch_dev, aiy_dist_forward_batch_dev): the paths' prices
// and per-path results on the device and their pinned copies, sized for the largest call seen
struct TransitionBlocks {
    DevBuf<double> rw;       // device [C][T+1] r, then [C][T] w
    DevBuf<int> res;         // device [2][C]: status, fail_t
    PinnedBuf<double> hrw;
    PinnedBuf<int> hres;
    int ensure(size_t C, size_t T) {  // (the entries bound C and T below 2^31: no overflow)
        AIY_TRY(rw.ensure(C * (2 * T + 1)));
        AIY_TRY(res.ensure(2 * C));
        AIY_TRY(hrw.ensure(C * (2 * T + 1)));
        return hres.ensure(2 * C);
    }
};
}  // namespace aiy

struct aiy_ws {
    template <class T>
    using Dev = aiy::DevBuf<T>;
    using u64 = aiy::u64;
    int64_t N = 0, Na = 0, Nl = 1;
    int dev = 0;
    // search knobs (aiy_ws_set_search)
    int coarse = 512;
    int CK = 1024;
    int variant = -1;  // -1: by size (see bell_args); EGM knobs: bits 18-20 (egm_knob)
    // VFI scratch (ws_ensure_bell)
    Dev<double> EV;
    Dev<double2> T;
    Dev<float> T32;
    Dev<double> Dm, Dm8, Dt, Dm512, best0;
    Dev<int> idx0;
    Dev<int> mom;  // [N][Na] last sweep's argmax shift (tree kernel start-up heuristic)
    Dev<int> touched;
    Dev<double> dis;
    Dev<int> kf;
    // key of the cached kf table (feasible prefixes depend on r, w, a, s, L only)
    bool kf_ok = false;
    double kf_r = 0, kf_w = 0;
    const void* kf_a = nullptr;
    const void* kf_s = nullptr;
    const void* kf_L = nullptr;
    int64_t kf_Nl = 0;
    bool kf_lab = false;
    Dev<int> tree_perm;  // tree dispatch order for the cached kf (ws_tree_perm)
    int perm_slots = 0;
    long long perm_key = 0;
    Dev<int> kf_last;    // [Nl][N][ntile] kf of each tile's last state (ws_tree_perm)
    // disutility per labour level, cached with the key below (aiy_ws_invalidate resets)
    bool dis_ok = false;
    const void* dis_L = nullptr;
    int64_t dis_Nl = 0;
    double dis_psi = 0, dis_eta = 0;
    // small-grid one-launch sweep (bellman_wide_kernels.hip; aiy_ws_set_wide): used when
    // Na <= wide_max (-1: the default bound) with `wide_S` splits of `wide_NW` waves (0: by size)
    int wide_max = -1, wide_S = 0, wide_NW = 0, wide_SB = 0;
    bool cu_exclusive = false;  // aiy_ws_set_cu_exclusive
    // A9 chains (aiy_ws_set_sim): -1 by size, 0 the serial kernels, 1 / 2 the speculative-
    // segment chain (one workgroup / spread over 16) whenever it applies; its scratch
    int sim_par = -1;
    Dev<double> sim_kbuf;
    Dev<u64> wdiff;          // device [2][2*kDiffSlots]: the set not current is zero
    int wcur = 0;            // the set the last wide sweep wrote
    Dev<unsigned> wcnt;      // device [N·ntile] per-tile arrival counters (zero)
    Dev<u64> wpart;          // device [N·ntile][S][64][2] partial bests
    bool last_wide = false;  // the last VFI sweep on this workspace was wide
    u64* vdiff = nullptr;    // (not owned) the diff slots the last VFI sweep wrote
    bool perm_ok = false;
    Dev<int> partial;
    Dev<u64> diff;           // device [2*kDiffSlots] {max bits, any}   (ws_ensure_diff)
    Dev<u64> hitcount;       // device [kHitcountLen]
    Dev<long long> trace;    // device [16 * units] (instrumentation; ws_ensure_trace)
    bool tracing = false;
    aiy::PinnedBuf<u64> hdiff;  // pinned host [2*kDiffSlots + 4]
    // histogram scratch (A10)
    Dev<int> d_key;
    Dev<int> d_off;  // [N][Na+1] run offsets of the policy (the plan)
    Dev<double> d_wr, d_mass, d_part;
    aiy::SlotRings dist;  // speculative histogram iteration
    // generic scratch used by the EGM / distribution / simulation kernels
    Dev<double> g0, g1, g2;
    Dev<unsigned> gi;  // [16] flag words (EGM, histogram)
    // speculative solves (aiy_ws_set_speculation): batches of up to spec_max steps
    int spec_max = 16;
    aiy::SpecRings spec;
    aiy::SlotRings egm;
    // chained EGM solve (Na > 1,024): the second â / c̃ pair (step parity)
    Dev<double> egm_x2, egm_y2;
    Dev<int> egm_seg;  // [N][Na] interp1 segments of the last step (hints), -1 = none
    aiy::BatchBlocks batch;
    // batched multi-rate EGM solve (aiy_egm_solve_batch_dev; aiy_ws_set_egm_batch): the one-launch
    // path from egm_batch_min candidates on (-1: egm_batch_min_c, 0: never), its blocks, and how
    // often each path ran on this workspace (aiy_ws_egm_batch_counts)
    int egm_batch_min = -1;
    aiy::EgmBatchBlocks egm_batch;
    int64_t egm_batch_launches = 0, egm_batch_fallbacks = 0;
    // batched multi-rate labour VFI solve (aiy_labor_vfi_solve_batch_dev; aiy_ws_set_labor_batch):
    // one launch per sweep over all candidates from labor_batch_min candidates on (0: the
    // default, kLaborBatchMinC), its blocks, and how often each path ran on this workspace
    int labor_batch_min = 0;
    aiy::LaborBatchBlocks labor_batch;
    int64_t labor_batch_solves = 0, labor_batch_fallbacks = 0;
    // batched histogram solve (aiy_dist_stationary_batch_dev; aiy_ws_set_dist_batch): the
    // one-launch path from dist_batch_min candidates on (-1: kDistBatchMinC, 0: never), its
    // blocks, and how often each path ran on this workspace (aiy_ws_dist_batch_counts)
    int dist_batch_min = -1;
    aiy::DistBatchBlocks dist_batch;
    int64_t dist_batch_launches = 0, dist_batch_fallbacks = 0;
    aiy::TransitionBlocks transition;
    // timing of the dominant kernel
    bool timing = false, count_hits = false;
    aiy::Events ev_start, ev_stop;
    int ev_used = 0;
    double tot_ms = 0;
    int64_t launches = 0;
};

namespace aiy {
inline bool egm_knob(const aiy_ws* ws, int bit) { return ws->variant >= 0 && (ws->variant & bit); }
struct BellCall {
    bool labor = false;
    int64_t Nl = 1;
    const double* L = nullptr;
    double psi = 0, eta = 0;
    const double* v_old = nullptr;
    const double* a = nullptr;
    const double* s = nullptr;
    const double* P = nullptr;
    double r = 0, w = 0, beta = 0, sigma = 0;
    const int* hint = nullptr;
    int mode = 0;
    bool keep_incoming = true;
    double* v_new = nullptr;
    int* idx = nullptr;
    double* pk = nullptr;
    double* pl = nullptr;
    double* pc = nullptr;
    double* diff_out = nullptr;
    void* prev_diff_out = nullptr;  // [2] u64: the previous sweep's folded {max bits, any}
};
int ws_ensure_bell(aiy_ws* ws, size_t partial_slots);
// diff (device slots) and hdiff (their pinned copy + 4 words): VFI, EGM and histogram paths
int ws_ensure_diff(aiy_ws* ws);
// the trace buffer: 16 words per unit; *fresh (nullable) = newly allocated (contents undefined)
int ws_ensure_trace(aiy_ws* ws, int64_t units, bool* fresh = nullptr);
inline int64_t ws_trace_units(const aiy_ws* ws) { return (int64_t)(ws->trace.cap() / 16); }
int ws_timing_begin(aiy_ws* ws, hipStream_t st);
int ws_timing_end(aiy_ws* ws, hipStream_t st);
int ws_timing_drain(aiy_ws* ws);
int ws_dispatch_arm(aiy_ws* ws);
void ws_dispatch_commit(aiy_ws* ws);
int ws_read_diff(aiy_ws* ws, hipStream_t st, double* d);
int bell_sweep_dev(aiy_ws* ws, const BellCall& c, hipStream_t st);
int bell_solve_dev(aiy_ws* ws, BellCall c, double* v_a, double* v_b, double tol,
                   int64_t max_iter, int64_t* iters, int* out_new, hipStream_t st);
int bell_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w, double* v_a,
                         double* v_b, const double* a, const double* s, const double* P,
                         double beta, double sigma, double tol, int64_t max_iter, int use_hint,
                         int* idx, double* pk, double* pc, int64_t* iters, int* which,
                         hipStream_t st);
// A3 at C candidate rates: one small-grid launch per sweep over all candidates still running
// where the shape takes the one-launch sweep and C reaches the workspace's threshold, else one
// bell_solve_dev after another (same results).  Arrays as BellArgs' batch layout; r, w, iters,
// which: host [C].
constexpr int kLaborBatchMinC = 2;  // default dispatch threshold
int bell_labor_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                               double* v_a, double* v_b, const double* a, const double* s,
                               const double* P, const double* L, double beta, double sigma,
                               double psi, double eta, double tol, int64_t max_iter, int use_hint,
                               int* lin, double* pk, double* pl, double* pc, int64_t* iters,
                               int* which, hipStream_t st);
int launch_reduce_slots(const unsigned long long* slots, void* out, hipStream_t st);
double fold_slots_host(const unsigned long long* h);
int launch_disutility(const double* L, int Nl, double psi, double eta, double* dis,
                      hipStream_t st);
}  // namespace aiy
