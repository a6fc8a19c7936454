// The Bellman drivers behind the device tier: one sweep (A1/A3: argument set-up, the cached
// feasible prefixes and dispatch order, the small-grid and tree paths), the A2 solve loop and
// the two batched multi-rate solves.  Host code only; kernels live in bellman*_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aiy_common.hpp"
#include "spec_loop.hpp"
#include "tree_perm.hpp"
#include "wide_batch.hpp"
#include "ws.hpp"

namespace aiy {

// ---------------------------------------------------------------------------- Bellman sweep
bool tree_perm_eligible(const BellArgs& A);
int ws_tree_perm(aiy_ws* ws, const BellArgs& A, hipStream_t st);

// the CRRA power the screened kernels multiply out: sigma - 1 for integer sigma in [2, 9], else
// 0 (plain sweeps)
static int bell_np(double sigma) {
    return is_int_ge(sigma, 2.0) && sigma <= 9.0 ? (int)sigma - 1 : 0;
}

// the small-grid kernels' flag word (AIY_WIDE_FLAGS: A/B tooling, tools/wide_tune.py)
static int wide_flags() {
    const char* fl = getenv("AIY_WIDE_FLAGS");
    return fl ? atoi(fl) : kWideDefaultFlags;
}

// disutility per level into ws->dis: cached while (L, Nl, psi, eta) are unchanged (a launch per
// sweep otherwise — a dependent launch in the small-grid sweep's one-launch chain)
static int ws_disutility(aiy_ws* ws, const double* L, int64_t Nl, double psi, double eta,
                         hipStream_t st) {
    if (ws->dis_ok && ws->dis_L == L && ws->dis_Nl == Nl && ws->dis_psi == psi &&
        ws->dis_eta == eta)
        return AIY_OK;
    AIY_TRY(launch_disutility(L, (int)Nl, psi, eta, ws->dis, st));
    ws->dis_ok = true;
    ws->dis_L = L; ws->dis_Nl = Nl; ws->dis_psi = psi; ws->dis_eta = eta;
    return AIY_OK;
}

// validation, the kernel arguments of one sweep, and the cached feasible prefixes
static int bell_args(aiy_ws* ws, const BellCall& c, BellArgs& A, hipStream_t st) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (!c.v_old || !c.a || !c.s || !c.P || !c.v_new || !c.idx)
        return fail(AIY_BAD_ARG, "NULL device pointer");
    if (c.labor && (!c.L || c.Nl < 1 || c.Nl > ws->Nl))
        return fail(AIY_BAD_ARG, "labour sweep needs labor_choice and 1 <= Nl <= workspace Nl");
    if (!(c.beta == c.beta) || !(c.r == c.r) || !(c.w == c.w) || !(c.sigma == c.sigma))
        return fail(AIY_NON_FINITE, "non-finite scalar argument");
    A = BellArgs{};
    A.N = (int)ws->N;
    A.Na = (int)ws->Na;
    A.Nl = c.labor ? (int)c.Nl : 1;
    A.labor = c.labor;
    A.keep_incoming = c.keep_incoming;
    A.np = bell_np(c.sigma);
    if (c.mode == 1 && A.np == 0)
        return fail(AIY_BAD_ARG, "screened sweep (mode 1) needs integer sigma in [2, 9]");
    A.coarse = ws->coarse;
    A.CK = ws->CK;
    // default geometry by size (measured at Na = 400: 2 cooperating waves per tile 10 % faster;
    // at Na = 20,000 one wave per tile, XCD-aware tile order: 44.3 vs 45.9 us).  Labour at
    // Na <= 4096: 4 waves per tile with the first superblock's passing 8-blocks dealt
    // round-robin (bit 12) — Na = 400 sweep 58.1 -> 41.8 us, 1,000: 61.8 -> 54.8, 2,000:
    // 81.5 -> 70.3 (profiles/r02c_s6_*); A1 is neutral to it (16.4 us either way)
    // (Na > 4096: bit 13, tiles in descending j, is faster in a solve's early sweeps — sweep 25:
    // 34.9 vs 35.8 us — and slower once the policy has settled — sweep 100: 33.6 vs 32.8 us,
    // whole solve to tol 9.37 vs 8.99 ms — so the order stays row-major, XCD-contiguous (16)).
    // Round 4, A1 at Na > 4096: bit 11 (each XCD's cheapest 2 x 128 tiles dispatched last, the
    // rest row-major) over 16 alone, three alternating runs on one box: step 39.3 -> 36.3 us,
    // solve to tol 8.74 -> 8.63 ms; heaviest-first (bit 6) 37.6 us / 8.75 ms; narrower tiles
    // (bit 13) slower, 40.6 / 39.3 us (profiles/r04_g7_order_ab.txt).  Two one-wave tiles per
    // workgroup (bits 16-17 = 1) on top: 36.5 -> 36.0 us, solve 8.68 -> 8.59 ms; four: 36.3 us,
    // eight: 47 us (profiles/r04_g9_pack_ab.txt).  Bit 21 (the start's drift extrapolated from
    // the last two shifts): A1 36.1 -> 35.6 us, labour 0.285 -> 0.276 ms; neutral at Na = 400
    // (profiles/r04_g27_*, r04_g28_*).  Bit 23 (the hint's window reduced to the hint when the
    // extrapolated window is used) on top for A1: 36.2 -> 35.75 us (profiles/r04_g33_*); bit 24
    // (no hint evaluation then at all): kernel 30.9 -> 30.6 us, step 35.7 -> 35.6 (r04_g36_*)
    const int var = ws->variant >= 0 ? ws->variant
                    : ws->Na <= 4096 ? (c.labor ? var_waves(2) | kVarDealBlocks : var_waves(1))
                    : (c.labor ? kVarXcdOrder | kVarDriftExtrap
                               : kVarXcdOrder | kVarPermCheapLast | var_pack(1) | kVarDriftExtrap |
                                     kVarHintAlone | kVarNoHintEval);
    A.variant = var;
    A.ev_mfma = bell_ev_mfma(A.N, ws->variant);
    // (variant bit 13) one-wave tiles of tw < 64 states, tw = ceil(N·Na / (3 waves × 1,024
    // SIMDs)): every SIMD holds three tiles instead of two or three (the 3-wave SIMDs end the
    // launch, tools/tree_trace.py); lanes tw..63 idle.  Work split only.
    A.tw = 0;
    if ((var & kVarNarrowTiles) && !c.labor && (var & kVarGeometryMask) == 0) {
        const int64_t tw = (ws->N * ws->Na + 3 * 1024 - 1) / (3 * 1024);
        A.tw = (int)std::max<int64_t>(16, std::min<int64_t>(64, tw));
        if (A.tw == 64) A.tw = 0;
    }
    A.r = c.r;
    A.w = c.w;
    A.beta = c.beta;
    A.sigma = c.sigma;
    A.v_old = c.v_old;
    A.a = c.a;
    A.s = c.s;
    A.P = c.P;
    A.L = c.labor ? c.L : nullptr;
    A.hint = c.hint;
    AIY_TRY(ws_ensure_bell(ws, bell_partial_slots(A)));
    A.dis = c.labor ? ws->dis : nullptr;
    A.EV = ws->EV;
    A.T = ws->T;
    A.tree = (var & kVarChunked) == 0;
    A.T32 = (A.tree || (var & kVarFp64Screen)) ? nullptr : ws->T32;
    A.Dm = A.tree ? nullptr : ws->Dm;
    A.Dm8 = A.tree ? ws->Dm8 : nullptr;
    A.Dt = A.tree ? ws->Dt : nullptr;
    A.Dm512 = A.tree ? ws->Dm512 : nullptr;
    A.nb = (int)((ws->Na + 63) / 64);
    A.nb8 = (int)((ws->Na + 7) / 8);
    A.nb512 = (int)((ws->Na + 511) / 512);
    A.best0 = ws->best0;
    A.idx0 = ws->idx0;
    A.mom = ws->mom;
    A.partial = ws->partial;
    A.touched = ws->touched;
    A.hitcount = ws->count_hits ? ws->hitcount : nullptr;
    A.trace = nullptr;
    if (ws->tracing) {
        bool fresh;  // a record per quad tile: 16 states
        AIY_TRY(ws_ensure_trace(ws, (int64_t)ws->N * ((ws->Na + 15) / 16), &fresh));
        if (fresh) AIY_HIP(hipMemset(ws->trace, 0, ws->trace.cap() * sizeof(long long)));
        A.trace = ws->trace;
    }
    A.v_new = c.v_new;
    A.idx = c.idx;
    A.pk = c.pk;
    A.pl = c.pl;
    A.pc = c.pc;
    A.diff = ws->diff;
    A.fold = (unsigned long long*)c.prev_diff_out;
    if (c.labor) AIY_TRY(ws_disutility(ws, c.L, c.Nl, c.psi, c.eta, st));
    // feasible prefixes: cached while (r, w, a, s, L) are unchanged (aiy_ws_invalidate resets)
    bool kf_new;
    AIY_TRY(ws->kf.ensure((size_t)A.Nl * A.N * A.Na, &kf_new));
    if (kf_new) ws->kf_ok = false;
    A.kf = ws->kf;
    bool fresh = ws->kf_ok && ws->kf_r == c.r && ws->kf_w == c.w && ws->kf_a == c.a &&
                 ws->kf_s == c.s && ws->kf_L == A.L && ws->kf_Nl == A.Nl && ws->kf_lab == A.labor;
    if (!fresh) {
        AIY_TRY(launch_bell_kf(A, st));
        ws->kf_ok = true;
        ws->kf_r = c.r; ws->kf_w = c.w; ws->kf_a = c.a; ws->kf_s = c.s; ws->kf_L = A.L;
        ws->kf_Nl = A.Nl; ws->kf_lab = A.labor;
        ws->perm_ok = false;
    }
    A.perm = nullptr;
    A.perm_slots = 0;
    if (tree_perm_eligible(A)) {
        const long long key = (long long)A.tw * (1ll << 31) +
                              (A.variant & kVarPermKeyMask);
        if (!ws->perm_ok || ws->perm_key != key) {
            AIY_TRY(ws_tree_perm(ws, A, st));
            ws->perm_key = key;
        }
        A.perm = ws->tree_perm;
        A.perm_slots = ws->perm_slots;
    }
    return AIY_OK;
}

// The dispatch permutation of the one-wave-per-tile A1 tree launch: the order is tree_perm.hpp's
// (a pure function of the tiles' costs); here the costs are fetched and the order uploaded.
bool tree_perm_eligible(const BellArgs& A) {
    return (A.variant & kVarPermMask) && A.tree && A.C <= 1 && A.np >= 1 && A.np <= 8 &&
           (A.variant & kVarGeometryMask) == 0;
}
static int ws_upload_perm(aiy_ws* ws, const std::vector<int>& perm, hipStream_t st) {
    AIY_TRY(ws->tree_perm.ensure(perm.size()));
    AIY_HIP(hipMemcpyAsync(ws->tree_perm, perm.data(), perm.size() * sizeof(int),
                           hipMemcpyHostToDevice, st));
    AIY_HIP(hipStreamSynchronize(st));
    ws->perm_ok = true;
    ws->perm_slots = (int)perm.size();
    return AIY_OK;
}
int ws_tree_perm(aiy_ws* ws, const BellArgs& A, hipStream_t st) {
    const int N = A.N, Na = A.Na, TW = bell_tile_width(A, 1), ntile = (Na + TW - 1) / TW;
    // only each tile's last state's prefixes cross to the host (not all of kf)
    const int rows = A.Nl * N;
    AIY_TRY(ws->kf_last.ensure((size_t)rows * ntile));
    std::vector<int> kl((size_t)rows * ntile);  // [labour level][row][tile]
    AIY_TRY(launch_kf_tile_last(A.kf, rows, Na, TW, ntile, ws->kf_last, st));
    AIY_HIP(hipMemcpyAsync(kl.data(), ws->kf_last, kl.size() * sizeof(int),
                           hipMemcpyDeviceToHost, st));
    AIY_HIP(hipStreamSynchronize(st));
    return ws_upload_perm(ws,
                          bell_tree_hybrid(A)
                              ? tree_perm_hybrid_order(kl, N, ntile, A.Nl, bell_tree_coop_per_xcd(A))
                              : tree_perm_order(kl, N, ntile, A.Nl, bell_tree_pack(A),
                                                (A.variant & kVarPermHeavy) != 0),
                          st);
}

// The small-grid one-launch sweep (bellman_wide_kernels.hip) and its geometry.  Default: every
// screened sweep at Na <= 1,536 (A1) / 2,048 (labour) unless a tree geometry was asked for
// (variant >= 0 without bit 25); aiy_ws_set_wide overrides the bound and the geometry.
// Measured (tools/wide_tune.py, profiles/r05_wide_tune.jsonl; sweeps 11-60 from v = 0, per
// sweep, tree = table + tree launch): A1 Na = 400 7.7 vs 13.8 us, 1,000 10.2 vs 16.4, 2,048
// 16.7 vs 16.5 (a tie: the tree from there); labour Na = 400 17 vs 32 us, 1,000 25 vs 52, 2,000
// 56 vs 60.  One workgroup per tile (splits = 1): the cross-workgroup hand-off (sc1 partials,
// an arrival counter) costs more than the extra workgroups save at every size measured.
static bool wide_pick(const aiy_ws* ws, const BellArgs& A, int* S, int* NW, int* SB) {
    if (A.np < 1 || A.np > 8 || A.C > 1 || A.ev_mfma || A.Nl > kWideMaxNl) return false;
    const int vmax = ws->wide_max >= 0 ? ws->wide_max : (A.labor ? 2048 : 1536);
    if (A.Na > vmax) return false;
    if (ws->variant >= 0 && !(ws->variant & kVarWide)) return false;
    // states per wave: labour 16 up to Na = 512, then 32 (profiles/r05_wide_ab.txt, r05_g52:
    // Na = 1,000 30.8 -> 21.8 us, 2,000 69.9 -> 56.4); A1 32 up to 1,024, then 64
    const int sb = ws->wide_SB > 0 ? ws->wide_SB
                                   : (A.labor ? (A.Na <= 512 ? 16 : 32) : (A.Na <= 1024 ? 32 : 64));
    const int nw = ws->wide_NW > 0 ? ws->wide_NW : 8;
    const int s = ws->wide_S > 0 ? ws->wide_S : 1;
    if (bell_wide_lds(A.Na, s, nw) > kWideMaxLds) return false;
    *S = s;
    *NW = nw;
    *SB = sb;
    return true;
}

static int bell_sweep_wide(aiy_ws* ws, BellArgs& A, int S, int NW, int SB, hipStream_t st) {
    const int ntile = (int)((ws->Na + SB - 1) / SB);
    const size_t items = (size_t)ws->N * ntile;
    bool fresh;
    AIY_TRY(ws->wdiff.ensure(4 * (size_t)kDiffSlots, &fresh));
    if (fresh) {
        AIY_HIP(hipMemsetAsync(ws->wdiff, 0, 4 * kDiffSlots * sizeof(unsigned long long), st));
        ws->wcur = 0;
    }
    AIY_TRY(ws->wcnt.ensure(items, &fresh));
    if (fresh) AIY_HIP(hipMemsetAsync(ws->wcnt, 0, items * sizeof(unsigned), st));
    if (S > 1) AIY_TRY(ws->wpart.ensure(items * (size_t)S * 64 * 2));
    unsigned long long* cur = ws->wdiff + (size_t)ws->wcur * 2 * kDiffSlots;
    unsigned long long* nxt = ws->wdiff + (size_t)(ws->wcur ^ 1) * 2 * kDiffSlots;
    if (A.fold && !ws->last_wide) {  // the previous sweep's slots are the table path's
        AIY_TRY(launch_reduce_slots(ws->diff, A.fold, st));
        A.fold = nullptr;
    }
    A.diff = nxt;  // zero (the set not current); block 0 folds and clears `cur`
    A.trace = nullptr;
    if (ws->tracing) {  // one 64-word record per block (instrumentation)
        AIY_TRY(ws_ensure_trace(ws, ((int64_t)items + 7) / 8 * 8 * S * 4));  // (16-word units)
        AIY_HIP(hipMemsetAsync(ws->trace, 0, ws->trace.cap() * sizeof(long long), st));
        A.trace = ws->trace;
    }
    AIY_TRY(ws_dispatch_arm(ws));
    const int rc = launch_bell_wide(A, S, NW, SB, cur, ws->wcnt, ws->wpart, wide_flags(),
                                    ws->cu_exclusive ? kExclusiveLds : 0, st);
    ws_dispatch_commit(ws);
    AIY_TRY(rc);
    ws->wcur ^= 1;
    ws->vdiff = nxt;
    ws->last_wide = true;
    return AIY_OK;
}

int bell_sweep_dev(aiy_ws* ws, const BellCall& c, hipStream_t st) {
    BellArgs A;
    AIY_TRY(bell_args(ws, c, A, st));
    // mode 2 / variant bit 10: the exhaustive scan (one launch after the table, outputs written
    // by the scan itself); otherwise the bound tree (or the chunked screen, variant bit 3)
    const bool exhaustive = c.mode == 2 || A.np == 0 || (A.variant & kVarExhaustive);
    const bool screened = !exhaustive;
    int wS = 0, wNW = 0, wSB = 0;
    if (screened && wide_pick(ws, A, &wS, &wNW, &wSB)) {  // small grids: one launch per sweep
        AIY_TRY(bell_sweep_wide(ws, A, wS, wNW, wSB, st));
        if (c.diff_out) AIY_TRY(launch_reduce_slots(ws->vdiff, c.diff_out, st));
        return AIY_OK;
    }
    if (ws->last_wide && A.fold) {  // the previous sweep's slots are the wide path's
        AIY_TRY(launch_reduce_slots(ws->vdiff, A.fold, st));
        A.fold = nullptr;
    }
    ws->last_wide = false;
    ws->vdiff = ws->diff;
    AIY_TRY(launch_bell_table(A, st));  // also clears the diff slots
    if (!screened) A.coarse = 0, A.hint = nullptr;
    if (screened && A.tree) {
        // tree screen: the hint (or, cold, the init kernel's candidate) sets the first bar;
        // the tree kernel writes the outputs itself
        if (!A.hint) AIY_TRY(launch_bell_init(A, st));
        AIY_TRY(ws_dispatch_arm(ws));  // events recorded by the dispatch itself
        const int rc = launch_bell_tree(A, st);
        ws_dispatch_commit(ws);
        AIY_TRY(rc);
    } else if (screened) {
        AIY_TRY(launch_bell_init(A, st));
        AIY_TRY(ws_timing_begin(ws, st));
        AIY_TRY(launch_bell_screen(A, st));
        AIY_TRY(ws_timing_end(ws, st));
        AIY_TRY(launch_bell_merge(A, 1, st));
    } else {
        AIY_TRY(ws_timing_begin(ws, st));
        AIY_TRY(launch_bell_plain(A, st));
        AIY_TRY(ws_timing_end(ws, st));
    }
    if (c.diff_out) AIY_TRY(launch_reduce_slots(ws->diff, c.diff_out, st));
    return AIY_OK;
}

// read {max|Δ| bits, any} from the workspace diff word (synchronises the stream)
int ws_read_diff(aiy_ws* ws, hipStream_t st, double* d) {
    const unsigned long long* sl = ws->vdiff ? ws->vdiff : ws->diff;  // the last sweep's slots
    AIY_HIP(hipMemcpyAsync(ws->hdiff, sl, 2 * kDiffSlots * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st));
    AIY_HIP(hipStreamSynchronize(st));
    *d = fold_slots_host(ws->hdiff);
    return AIY_OK;
}

// A2 with speculative batches.  The one-sweep-at-a-time loop pays a stream synchronisation per
// sweep to read max|Δv| (at the script's Na = 400 that round trip costs more than the sweep).
// Here sweeps are enqueued m at a time: sweep g reads ring slot (g−1) mod R and writes slot
// g mod R (R = 2·spec_max + 1 value buffers), its policies go to set g mod 2·spec_max, its folded
// diff to its own slot, and one D2H read per batch finds the first sweep below tol.  Sweeps
// are deterministic and each depends only on its predecessor, so sweeps 1..g* are exactly the
// ones the plain loop runs; later sweeps of the batch are discarded and the ring still holds
// v_new(g*), v_old = v(g*−1) and the policies of g*.  m follows the observed geometric decay
// of the diff (sweeps still needed to reach tol), capped at spec_max.
static int bell_solve_spec(aiy_ws* ws, BellCall c, double* v_a, double* v_b, double tol,
                           int64_t max_iter, int64_t* iters, int* out_new, hipStream_t st) {
    // rings sized for two batches in flight: v 2M + 1 (the stopping sweep's v_new and v_old
    // survive the next batch), idx / policies 2M, diff pairs 2M (indexed by sweep)
    const int M = ws->spec_max, R = 2 * M + 1, Rp = 2 * M, D = 2 * M;
    const size_t n = (size_t)ws->N * ws->Na;
    SpecRings& sp = ws->spec;
    if (sp.n != n || sp.m != M) {
        sp = SpecRings{};
        AIY_TRY(sp.v.ensure((size_t)R * n));
        AIY_TRY(sp.idx.ensure((size_t)Rp * n));
        AIY_TRY(sp.pol.ensure((size_t)Rp * 3 * n));
        AIY_TRY(sp.diff.ensure(2 * (size_t)D));
        AIY_TRY(sp.hdiff.ensure(2 * 2 * (size_t)D));
        AIY_TRY(sp.ev.create(2, hipEventDisableTiming));
        sp.n = n;
        sp.m = M;
    }
    auto vslot = [&](int64_t g) { return sp.v + (size_t)(g % R) * n; };
    auto islot = [&](int64_t g) { return sp.idx + (size_t)(g % Rp) * n; };
    auto pslot = [&](int64_t g, int q) { return sp.pol + ((size_t)(g % Rp) * 3 + q) * n; };
    auto dslot = [&](int64_t g) { return sp.diff + 2 * (size_t)(g % D); };
    const size_t vb = n * sizeof(double);
    // slot 0 = v_old of sweep 1; slot 1 = the incoming v_new buffer (the labour sweep's
    // keep-incoming rule reads it on sweep 1)
    AIY_HIP(hipMemcpyAsync(vslot(0), v_a, vb, hipMemcpyDeviceToDevice, st));
    AIY_HIP(hipMemcpyAsync(vslot(1), v_b, vb, hipMemcpyDeviceToDevice, st));
    const int* first_hint = c.hint;
    double* const upk = c.pk;
    double* const upc = c.pc;
    double* const upl = c.pl;
    int* const uidx = c.idx;
    if (c.labor) {
        // Labor_VFI.m:85: a state with no feasible choice keeps its incoming policies (the
        // kernels do not write them).  The plain loop reuses the caller's buffers, so those
        // entries stay the caller's; every ring slot starts as a copy of them to match
        // (feasibility depends on (r, w, grids) only, so it is fixed within a solve).
        for (int q = 0; q < Rp; ++q) {
            AIY_HIP(hipMemcpyAsync(sp.idx + (size_t)q * n, uidx, n * sizeof(int),
                                   hipMemcpyDeviceToDevice, st));
            double* const src[3] = {upk, upc, upl};
            for (int p = 0; p < 3; ++p)
                if (src[p])
                    AIY_HIP(hipMemcpyAsync(sp.pol + ((size_t)q * 3 + p) * n, src[p], vb,
                                           hipMemcpyDeviceToDevice, st));
        }
    }
    // Batches of m sweeps, each ending with a D2H copy of the diff pairs and an event; two in
    // flight: the host reads batch k while batch k+1 runs, so the device never waits for a read
    // (spec_loop.hpp)
    int64_t last = 0;   // the last sweep enqueued
    int64_t folded = 0;  // the last sweep whose pair a reduce launch folded (its batch's end)
    auto sweep = [&](int64_t g) -> int {
        c.hint = (g == 1) ? first_hint : islot(g - 1);
        c.keep_incoming = (g == 1);
        c.v_old = vslot(g - 1);
        c.v_new = vslot(g);
        c.idx = islot(g);
        c.pk = upk ? pslot(g, 0) : nullptr;
        c.pc = upc ? pslot(g, 1) : nullptr;
        c.pl = upl ? pslot(g, 2) : nullptr;
        // sweep g's {max bits, any} lands in pair g: folded by sweep g+1's table kernel, or by
        // the reduce launch after the batch's last sweep
        c.prev_diff_out = (g - 1 != folded) ? dslot(g - 1) : nullptr;
        last = g;
        return bell_sweep_dev(ws, c, st);
    };
    auto flush = [&](int hb) -> int {
        AIY_TRY(launch_reduce_slots(ws->vdiff, dslot(last), st));
        folded = last;
        AIY_HIP(hipMemcpyAsync(sp.hdiff + (size_t)hb * 2 * D, sp.diff,
                               2 * (size_t)D * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               st));
        AIY_HIP(hipEventRecord(sp.ev[hb], st));
        return AIY_OK;
    };
    auto wait = [&](int hb) { return wait_event(sp.ev[hb]); };
    auto read = [&](int64_t g, int hb, double* d) -> int {
        const unsigned long long* h = sp.hdiff + (size_t)hb * 2 * D + 2 * (g % D);
        if (h[1]) std::memcpy(d, &h[0], sizeof *d);  // {max|Δ| bits, any non-NaN}; else NaN
        return AIY_OK;
    };
    SpecResult S;
    AIY_TRY(spec_loop(M, max_iter, tol, &S, sweep, flush, wait, read,
                      [tol](double d) { return d < tol; }));  // Aiyagari_VFI.m:85-86
    const int64_t g = S.g, stop = S.stop;
    // the plain loop leaves v_new in v_b after odd sweep counts (ping-pong from v_a)
    const int nw = (g & 1) ? 1 : 0;
    double* vnew = nw ? v_b : v_a;
    double* vold = nw ? v_a : v_b;
    AIY_HIP(hipMemcpyAsync(vnew, vslot(g), vb, hipMemcpyDeviceToDevice, st));
    // exhausted: v_old = v_new after the last sweep (:88); else the previous iterate
    AIY_HIP(hipMemcpyAsync(vold, stop ? vslot(g - 1) : vslot(g), vb, hipMemcpyDeviceToDevice, st));
    AIY_HIP(hipMemcpyAsync(uidx, islot(g), n * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (upk) AIY_HIP(hipMemcpyAsync(upk, pslot(g, 0), vb, hipMemcpyDeviceToDevice, st));
    if (upc) AIY_HIP(hipMemcpyAsync(upc, pslot(g, 1), vb, hipMemcpyDeviceToDevice, st));
    if (upl) AIY_HIP(hipMemcpyAsync(upl, pslot(g, 2), vb, hipMemcpyDeviceToDevice, st));
    *iters = g;
    *out_new = nw;
    return AIY_OK;
}

int bell_solve_dev(aiy_ws* ws, BellCall c, double* v_a, double* v_b, double tol,
                   int64_t max_iter, int64_t* iters, int* out_new, hipStream_t st) {
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    if (!c.idx) return fail(AIY_BAD_ARG, "NULL device pointer");
    if (ws && ws->spec_max > 1 && !c.diff_out) {
        // rings (two batches in flight, bell_solve_spec): 2M + 1 value buffers, 2M idx slots
        // and 2M x 3 policy slots, M = spec_max
        const size_t n = (size_t)ws->N * ws->Na, M2 = 2 * (size_t)ws->spec_max;
        const size_t bytes = ((M2 + 1) + 3 * M2) * n * sizeof(double) + M2 * n * sizeof(int);
        if (bytes <= ((size_t)8 << 30)) {
            int rc = bell_solve_spec(ws, c, v_a, v_b, tol, max_iter, iters, out_new, st);
            if (rc != AIY_NO_MEMORY) return rc;
            ws->spec = SpecRings{};  // no room for the rings: one synchronisation per sweep instead
        }
    }
    double* cur = v_a;
    double* nxt = v_b;
    const int* first_hint = c.hint;
    int64_t it;
    for (it = 1; it <= max_iter; ++it) {
        c.hint = (it == 1) ? first_hint : c.idx;
        c.keep_incoming = (it == 1);
        c.v_old = cur;
        c.v_new = nxt;
        AIY_TRY(bell_sweep_dev(ws, c, st));
        double d;
        AIY_TRY(ws_read_diff(ws, st, &d));
        if (d < tol) break;  // Aiyagari_VFI.m:85-86 (v_old keeps the previous iterate)
        std::swap(cur, nxt); // :88
    }
    if (it > max_iter) {  // loop exhausted: v_old = v_new after the last sweep
        it = max_iter;
        AIY_HIP(hipMemcpyAsync(nxt, cur, sizeof(double) * ws->N * ws->Na,
                               hipMemcpyDeviceToDevice, st));
        std::swap(cur, nxt);
    }
    *iters = it;
    *out_new = (nxt == v_a) ? 0 : 1;
    return AIY_OK;
}

// C candidate rates in lockstep (the two batched solves below): every sweep is one call of
// `sweep(g)` over all candidates still running, whose kernels apply the stopping test per
// candidate on the device and write the sweep a candidate stopped at into lb.stop; the host reads
// those flags once per m sweeps.  Sweep g reads buf[(g-1) & 1] and writes buf[g & 1] with
// buf[0] = v_a.  `prepare()` runs once, after r and w are on the device and before sweep 1 (the
// candidates' feasible prefixes); `slot_set(c, G)` is candidate c's device slot set of sweep G.
template <class Prepare, class Sweep, class SlotSet>
static int bell_lockstep(LockstepBlocks& lb, int64_t C, size_t n, const double* r, const double* w,
                         double tol, int64_t max_iter, int64_t m, double* v_a, double* v_b,
                         int64_t* iters, int* which, hipStream_t st, Prepare&& prepare,
                         Sweep&& sweep, SlotSet&& slot_set) {
    AIY_HIP(hipMemcpyAsync(lb.rw, r, C * sizeof(double), hipMemcpyHostToDevice, st));
    AIY_HIP(hipMemcpyAsync(lb.rw + C, w, C * sizeof(double), hipMemcpyHostToDevice, st));
    AIY_HIP(hipMemsetAsync(lb.stop, 0, C * sizeof(int), st));
    AIY_TRY(prepare());
    double* const buf[2] = {v_a, v_b};
    int64_t g = 0;
    bool all_stopped = false;
    while (!all_stopped && g < max_iter) {
        const int64_t gend = std::min(max_iter, g + m);
        while (g < gend) AIY_TRY(sweep(++g));
        AIY_HIP(hipMemcpyAsync(lb.hstop, lb.stop, C * sizeof(int), hipMemcpyDeviceToHost, st));
        AIY_HIP(hipStreamSynchronize(st));
        all_stopped = true;
        for (int64_t c = 0; c < C; ++c) all_stopped = all_stopped && lb.hstop[c] != 0;
    }
    // candidates still running after the last sweep G = max_iter: fold their sweep-G slots (the
    // stopping test of that sweep), else the loop was exhausted and v_old = v_new
    const int64_t G = g;
    if (!all_stopped) {
        for (int64_t c = 0; c < C; ++c)
            if (lb.hstop[c] == 0)
                AIY_HIP(hipMemcpyAsync(lb.hslots + c * 2 * kDiffSlots, slot_set(c, G),
                                       2 * kDiffSlots * sizeof(unsigned long long),
                                       hipMemcpyDeviceToHost, st));
        AIY_HIP(hipStreamSynchronize(st));
    }
    for (int64_t c = 0; c < C; ++c) {
        int64_t it = lb.hstop[c];
        if (it == 0) {
            const double d = fold_slots_host(lb.hslots + c * 2 * kDiffSlots);
            it = G;
            if (!(d < tol))  // exhausted: v_old = v_new after the last sweep
                AIY_HIP(hipMemcpyAsync(buf[(G - 1) & 1] + c * n, buf[G & 1] + c * n,
                                       n * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        iters[c] = it;
        which[c] = (int)(it & 1);
    }
    AIY_HIP(hipStreamSynchronize(st));
    return AIY_OK;
}

// Config 4 (BASELINE configs[3]): C candidate interest rates, each the A2 loop of
// Aiyagari_VFI.m:147-171 from its own v_old, solved together: every sweep is ONE table launch
// and ONE tree launch over all candidates still running (C·N·Na states), so the GPU sees C
// times the parallelism of one solve.  Each candidate stops at its own first sweep below tol
// (the table kernel applies :85 per candidate on the device and freezes it), so iteration
// counts, v_new, v_old and policies are exactly those of C separate solves.  The loop is
// bell_lockstep (`spec_max` sweeps per read of the stop flags): a candidate that stopped at g*
// holds v_new in buf[g* & 1].
int bell_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w, double* v_a,
                         double* v_b, const double* a, const double* s, const double* P,
                         double beta, double sigma, double tol, int64_t max_iter, int use_hint,
                         int* idx, double* pk, double* pc, int64_t* iters, int* which,
                         hipStream_t st) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (C < 1 || C > (1 << 20)) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 2^20 candidates");
    if (!r || !w || !v_a || !v_b || !a || !s || !P || !idx || !iters || !which)
        return fail(AIY_BAD_ARG, "NULL argument");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    for (int64_t c = 0; c < C; ++c)
        if (!(r[c] == r[c]) || !(w[c] == w[c])) return fail(AIY_NON_FINITE, "non-finite r or w");
    const size_t n = (size_t)ws->N * ws->Na;
    const int np = bell_np(sigma);
    if (np == 0 || C == 1) {
        // generic sigma (plain sweeps) or a single rate: one solve after another, same results
        for (int64_t c = 0; c < C; ++c) {
            BellCall bc{};
            bc.a = a; bc.s = s; bc.P = P; bc.r = r[c]; bc.w = w[c]; bc.beta = beta;
            bc.sigma = sigma; bc.idx = idx + c * n; bc.pk = pk ? pk + c * n : nullptr;
            bc.pc = pc ? pc + c * n : nullptr;
            bc.hint = use_hint ? idx + c * n : nullptr;
            AIY_TRY(bell_solve_dev(ws, bc, v_a + c * n, v_b + c * n, tol, max_iter, &iters[c],
                                   &which[c], st));
        }
        return AIY_OK;
    }
    if ((size_t)C * n > (size_t)INT32_MAX) return fail(AIY_BAD_SHAPE, "C*N*Na must fit int32");
    const int nb8 = (int)((ws->Na + 7) / 8), nb512 = (int)((ws->Na + 511) / 512);
    BatchBlocks& bb = ws->batch;
    if (bb.C != C) {
        bb = BatchBlocks{};
        AIY_TRY(bb.EV.ensure(C * n));
        AIY_TRY(bb.Dt.ensure(C * n));
        AIY_TRY(bb.Dm8.ensure((size_t)C * ws->N * nb8));
        AIY_TRY(bb.Dm512.ensure((size_t)C * ws->N * nb512));
        AIY_TRY(bb.best0.ensure(C * n));
        AIY_TRY(bb.idx0.ensure(C * n));
        AIY_TRY(bb.mom.ensure(C * n));
        AIY_HIP(hipMemset(bb.mom, 0, C * n * sizeof(int)));
        AIY_TRY(bb.kf.ensure(C * n));
        AIY_TRY(bb.slots.ensure((size_t)C * 2 * 2 * kDiffSlots));
        AIY_TRY(bb.ls.ensure((size_t)C));
        bb.C = C;
    }
    AIY_TRY(ws_ensure_bell(ws, 1));  // diff/hitcount scratch and events (single-rate buffers)
    BellArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.Nl = 1; A.labor = false; A.np = np;
    A.coarse = ws->coarse; A.CK = ws->CK;
    A.variant = ws->variant >= 0 ? ws->variant
                                   : (ws->Na <= 4096 ? 0 : kVarXcdOrder | kVarDriftExtrap);
    A.variant &= ~kVarGeometryMask;  // one state per lane, one wave per tile, tree screen
    A.ev_mfma = bell_ev_mfma(A.N, ws->variant);
    A.beta = beta; A.sigma = sigma; A.a = a; A.s = s; A.P = P;
    A.EV = bb.EV; A.Dt = bb.Dt; A.Dm8 = bb.Dm8; A.Dm512 = bb.Dm512;
    A.nb = (int)((ws->Na + 63) / 64); A.nb8 = nb8; A.nb512 = nb512;
    A.tree = true; A.best0 = bb.best0; A.idx0 = bb.idx0; A.kf = bb.kf; A.mom = bb.mom;
    A.hitcount = ws->count_hits ? ws->hitcount : nullptr;
    A.idx = idx; A.pk = pk; A.pc = pc; A.diff = bb.slots;
    A.C = (int)C; A.rv = bb.ls.rw; A.wv = bb.ls.rw + C; A.stop = bb.ls.stop;
    ws->kf_ok = false;  // (the single-rate kf cache is not this table)
    double* const buf[2] = {v_a, v_b};
    return bell_lockstep(
        bb.ls, C, n, r, w, tol, max_iter, std::max(ws->spec_max, 1), v_a, v_b, iters, which, st,
        [&] { return launch_bell_kf(A, st); },  // per-candidate feasible prefixes, once per solve
        [&](int64_t g) -> int {
            A.v_old = buf[(g - 1) & 1];
            A.v_new = buf[g & 1];
            A.parity = (int)(g & 1);
            A.hint = (g == 1 && !use_hint) ? nullptr : idx;
            if (A.ev_mfma) AIY_TRY(launch_bell_ev_mfma(A, st));
            AIY_TRY(launch_bell_table_batch(A, bb.slots, (int)g, tol, st));  // applies :85
            if (!A.hint) AIY_TRY(launch_bell_init(A, st));
            AIY_TRY(ws_timing_begin(ws, st));
            AIY_TRY(launch_bell_tree(A, st));
            return ws_timing_end(ws, st);
        },
        [&](int64_t c, int64_t G) {
            return bb.slots + ((size_t)c * 2 + (G & 1)) * 2 * kDiffSlots;
        });
}

// A3 at C candidate rates (one GE round of Aiyagari_Endogenous_Labor_VFI.m:166-219): each
// candidate the loop :64-122 from its own v_old / incoming v_new / policies, all candidates still
// running in ONE small-grid launch per sweep (bellman_wide_batch_kernels.hip).  The kernel runs
// each candidate's :115-118 test on the device (it folds the candidate's previous slot set and
// freezes the candidate), so iteration counts, v_new, v_old and policies are those of C separate
// solves.  The loop is bell_lockstep: buf[0] = v_a, so v_b holds every candidate's incoming v_new
// for sweep 1's keep-incoming rule (:85), and a candidate that stopped at g* holds v_new in
// buf[g* & 1].  Shapes the one-launch sweep does not take (wide_pick) and C below the workspace's
// threshold run one bell_solve_dev after another.
int bell_labor_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                               double* v_a, double* v_b, const double* a, const double* s,
                               const double* P, const double* L, double beta, double sigma,
                               double psi, double eta, double tol, int64_t max_iter, int use_hint,
                               int* lin, double* pk, double* pl, double* pc, int64_t* iters,
                               int* which, hipStream_t st) {
    if (!ws) return fail(AIY_BAD_ARG, "NULL workspace");
    if (!r || !w || !v_a || !v_b || v_a == v_b || !a || !s || !P || !L || !lin || !iters || !which)
        return fail(AIY_BAD_ARG, "NULL argument (or v_a == v_b)");
    if (C < 1 || C > (1 << 20)) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 2^20 candidates");
    if (max_iter < 1) return fail(AIY_BAD_ARG, "max_iter must be >= 1");
    for (int64_t c = 0; c < C; ++c)
        if (!std::isfinite(r[c]) || !std::isfinite(w[c]))
            return fail(AIY_NON_FINITE, "candidate %lld: non-finite r or w", (long long)c + 1);
    if (!(beta == beta) || !(sigma == sigma) || !(psi == psi) || !(eta == eta) || !(tol == tol))
        return fail(AIY_NON_FINITE, "non-finite scalar argument");
    const size_t n = (size_t)ws->N * ws->Na;
    const int64_t Nl = ws->Nl;
    if ((size_t)C * (size_t)Nl * n > (size_t)INT32_MAX)
        return fail(AIY_BAD_SHAPE, "C*Nl*N*Na must fit int32");
    BellArgs A{};
    A.N = (int)ws->N; A.Na = (int)ws->Na; A.Nl = (int)Nl; A.labor = true;
    A.np = bell_np(sigma);
    A.ev_mfma = bell_ev_mfma(A.N, ws->variant);
    int wS = 0, wNW = 0, wSB = 0;
    const int64_t min_c = ws->labor_batch_min > 0 ? ws->labor_batch_min : kLaborBatchMinC;
    if (C < min_c || !wide_pick(ws, A, &wS, &wNW, &wSB)) {
        for (int64_t c = 0; c < C; ++c) {
            BellCall bc{};
            bc.labor = true; bc.Nl = Nl; bc.L = L; bc.psi = psi; bc.eta = eta;
            bc.a = a; bc.s = s; bc.P = P; bc.r = r[c]; bc.w = w[c]; bc.beta = beta;
            bc.sigma = sigma; bc.idx = lin + c * n; bc.pk = pk ? pk + c * n : nullptr;
            bc.pl = pl ? pl + c * n : nullptr; bc.pc = pc ? pc + c * n : nullptr;
            bc.hint = use_hint ? lin + c * n : nullptr;
            AIY_TRY(bell_solve_dev(ws, bc, v_a + c * n, v_b + c * n, tol, max_iter, &iters[c],
                                   &which[c], st));
            ++ws->labor_batch_fallbacks;
        }
        AIY_HIP(hipStreamSynchronize(st));
        return AIY_OK;
    }
    LaborBatchBlocks& bb = ws->labor_batch;
    if (bb.C != C) {
        bb = LaborBatchBlocks{};
        AIY_TRY(bb.kf.ensure((size_t)C * Nl * n));
        AIY_TRY(bb.slots.ensure(wide_batch_set_off(C, 0, kDiffSlots)));
        AIY_TRY(bb.ls.ensure((size_t)C));
        bb.C = C;
    }
    AIY_TRY(ws_ensure_bell(ws, 1));  // dis / hitcount scratch and events (single-rate buffers)
    A.beta = beta; A.sigma = sigma; A.a = a; A.s = s; A.P = P; A.L = L; A.dis = ws->dis;
    A.r = r[0]; A.w = w[0];  // (C = 1: the kf kernel reads these)
    A.kf = bb.kf;
    A.hitcount = ws->count_hits ? ws->hitcount : nullptr;
    A.idx = lin; A.pk = pk; A.pl = pl; A.pc = pc;
    A.C = (int)C; A.rv = bb.ls.rw; A.wv = bb.ls.rw + C; A.stop = bb.ls.stop;
    const int flags = wide_flags();
    double* const buf[2] = {v_a, v_b};
    AIY_TRY(bell_lockstep(
        bb.ls, C, n, r, w, tol, max_iter, std::max(ws->spec_max, 1), v_a, v_b, iters, which, st,
        [&]() -> int {
            AIY_HIP(hipMemsetAsync(bb.slots, 0,
                                   wide_batch_set_off(C, 0, kDiffSlots) * sizeof(unsigned long long),
                                   st));
            AIY_TRY(ws_disutility(ws, L, Nl, psi, eta, st));
            return launch_bell_kf(A, st);  // per-candidate feasible prefixes, once per solve
        },
        [&](int64_t g) -> int {
            A.v_old = buf[(g - 1) & 1];
            A.v_new = buf[g & 1];
            A.keep_incoming = (g == 1);
            A.hint = (g == 1 && !use_hint) ? nullptr : lin;
            AIY_TRY(ws_dispatch_arm(ws));
            const int rc = launch_bell_wide_batch(A, wNW, wSB, bb.slots, bb.ls.stop, (int)g, tol,
                                                  flags, ws->cu_exclusive ? kExclusiveLds : 0, st);
            ws_dispatch_commit(ws);  // (the kernel applies :115-118)
            return rc;
        },
        [&](int64_t c, int64_t G) {
            return bb.slots + wide_batch_set_off(c, wide_batch_write_set(G), kDiffSlots);
        }));
    ++ws->labor_batch_solves;
    return AIY_OK;
}

}  // namespace aiy
