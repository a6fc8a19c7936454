// A3 at C candidate interest rates on small grids — one launch per sweep over every candidate
// still running (Aiyagari_Endogenous_Labor_VFI.m:166-219 at each rate of a GE round).
//
// The per-state arithmetic is the single-rate small-grid sweep's, shared with it
// (bell_wide_body.hpp: table into LDS, bar, 8-block screen, merge, output rules with the :85
// keep-incoming rule), run with one workgroup per (candidate, row, tile of SB states) and no split
// of the candidate range.  Around it this kernel only
//   - maps the block to (candidate c, tile item) and offsets the per-state arrays to c's blocks
//     ([C][N][Na]; kf [C][Nl][N][Na]; r, w from A.rv[c], A.wv[c]; L and dis shared);
//   - runs c's stop test (:115-118) on the device: every workgroup of c reads stop[c] and leaves
//     if it is set; otherwise it folds the slot set c's sweep g − 1 wrote (final: that launch has
//     ended) and leaves before writing anything when the fold is below tol — sweep g would
//     overwrite buffer g & 1, the v_old of a candidate that converged at g − 1.  c's first
//     workgroup records stop[c] = g − 1.  Every workgroup of c takes the same decision from the
//     same words, so none waits for another: no counters, no spinning, no hand-off.
//   - rotates three slot sets per candidate (wide_batch.hpp): write g mod 3, read (g − 1) mod 3,
//     c's first workgroup clears (g + 1) mod 3.
#include <hip/hip_runtime.h>

#include "aiy_common.hpp"
#include "bell_dev.hpp"
#include "bell_wide_body.hpp"
#include "bellman.hpp"
#include "wide_batch.hpp"

namespace aiy {

template <int NP, int NW>
__global__ __launch_bounds__(64 * NW) void bell_wide_batch_kernel(
    BellArgs A0, int ntile, int lsb, int bpc, unsigned long long* __restrict__ slots,
    int* __restrict__ stop, int g, double tol, int flags) {
    const WideBatchBlock wb = wide_batch_block((int)blockIdx.x, bpc);  // (block-uniform)
    const int c = wb.c, lane = threadIdx.x & 63;
    if (c >= A0.C) return;
    // the stop flag and the previous sweep's slots in one round of loads
    const int stopped = __hip_atomic_load(stop + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long* prev = slots + wide_batch_set_off(c, wide_batch_read_set(g), kDiffSlots);
    unsigned long long m = prev[2 * lane];
    const unsigned long long f = prev[2 * lane + 1];
    if (stopped) return;
    if (g > 1) {  // reduce_slots_kernel's fold, by every wave for itself
        const bool any = __ballot((f & 1ull) != 0ull) != 0ull;
        m = wave_max_u64_lane63(m);
        const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)m, 63);
        const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(m >> 32), 63);
        const double d = aiy_bitsd(((unsigned long long)hi << 32) | lo);
        if (any && d < tol) {  // NaN-only: no stop (:115)
            if (wb.item == 0 && threadIdx.x == 0)
                __hip_atomic_store(stop + c, g - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    if (wb.item == 0 && threadIdx.x < 64) {
        unsigned long long* nxt = slots + wide_batch_set_off(c, wide_batch_clear_set(g), kDiffSlots);
        nxt[2 * lane] = 0ull;
        nxt[2 * lane + 1] = 0ull;
    }
    // candidate c's blocks of every per-state array
    BellArgs A = A0;
    const size_t o = (size_t)c * A0.N * A0.Na;
    A.r = A0.rv[c];
    A.w = A0.wv[c];
    A.v_old += o;
    A.v_new += o;
    A.kf += o * A0.Nl;
    if (A.hint) A.hint += o;
    A.idx += o;
    if (A.pk) A.pk += o;
    if (A.pl) A.pl += o;
    if (A.pc) A.pc += o;
    A.diff = slots + wide_batch_set_off(c, wide_batch_write_set(g), kDiffSlots);
    A.fold = nullptr;
    A.trace = nullptr;
    A.C = 1;
    bell_wide_body<NP, true, NW>(A, ntile, 1, lsb, nullptr, nullptr, nullptr, flags, wb.item);
}

// ------------------------------------------------------------------------------ launcher
template <int NP, int NW>
static int wide_batch_geo(const BellArgs& A, int lsb, unsigned long long* slots, int* stop, int g,
                          double tol, int flags, size_t min_lds, hipStream_t st) {
    const int ntile = wide_batch_ntile(A.Na, 1 << lsb);
    const int bpc = wide_batch_bpc(A.N, ntile);
    const int grid = wide_batch_grid(A.C, bpc);
    if (grid < 1) return fail(AIY_BAD_SHAPE, "batched wide sweep: C*N*tiles must fit int32");
    const size_t lds = std::max(bell_wide_lds(A.Na, 1, NW), min_lds);
    if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
        AIY_TRY((raise_dynamic_lds<bell_wide_batch_kernel<NP, NW>>((int)kWideMaxLds)));
    launch_dispatch_timed(bell_wide_batch_kernel<NP, NW>, dim3(grid), dim3(64 * NW), lds, st, A,
                          ntile, lsb, bpc, slots, stop, g, tol, flags);
    return AIY_OK;
}
template <int NP>
static int wide_batch_w(const BellArgs& A, int NW, int lsb, unsigned long long* slots, int* stop,
                        int g, double tol, int flags, size_t min_lds, hipStream_t st) {
    // 4 or 8 waves (a 16-wave workgroup would cap the kernel at 128 registers, which it spills
    // at; the one-rate sweep's 16-wave tuning setting runs here with 8 — results do not depend
    // on it)
    if (NW == 4) return wide_batch_geo<NP, 4>(A, lsb, slots, stop, g, tol, flags, min_lds, st);
    return wide_batch_geo<NP, 8>(A, lsb, slots, stop, g, tol, flags, min_lds, st);
}

int launch_bell_wide_batch(const BellArgs& A, int NW, int SB, unsigned long long* slots, int* stop,
                           int sweep, double tol, int flags, size_t min_lds, hipStream_t st) {
    if (A.np < 1 || A.np > 8 || !A.labor || A.Nl < 1 || A.Nl > kWideMaxNl)
        return fail(AIY_BAD_ARG, "batched wide sweep: labour, integer sigma in [2, 9], Nl <= %d",
                    kWideMaxNl);
    if (A.C < 1 || !A.rv || !A.wv || !slots || !stop || sweep < 1)
        return fail(AIY_BAD_ARG, "batched wide sweep: candidates, their rates, slots and flags");
    if ((NW != 4 && NW != 8 && NW != 16) || (SB != 8 && SB != 16 && SB != 32 && SB != 64))
        return fail(AIY_BAD_ARG, "batched wide sweep: NW in {4, 8, 16}, SB in {8, ..., 64}");
    const int lsb = 31 - __builtin_clz((unsigned)SB);
    if (bell_wide_lds(A.Na, 1, NW) > kWideMaxLds)
        return fail(AIY_BAD_SHAPE, "batched wide sweep: the candidate range does not fit in LDS");
#define AIY_WBCASE(n)                                                                  \
    case n:                                                                            \
        rc = wide_batch_w<n>(A, NW, lsb, slots, stop, sweep, tol, flags, min_lds, st); \
        break;
    int rc = AIY_OK;
    switch (A.np) {
        AIY_WBCASE(1) AIY_WBCASE(2) AIY_WBCASE(3) AIY_WBCASE(4) AIY_WBCASE(5) AIY_WBCASE(6)
        AIY_WBCASE(7) AIY_WBCASE(8)
    }
#undef AIY_WBCASE
    AIY_TRY(rc);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
