// A1 / A3 on small grids at one interest rate — the whole Bellman sweep in ONE launch.  The
// workgroup body (and its description) is bell_wide_body.hpp, shared with the batched multi-rate
// kernel (bellman_wide_batch_kernels.hip); here: the kernel around it and its launcher.
#include <hip/hip_runtime.h>

#include "aiy_common.hpp"
#include "bell_dev.hpp"
#include "bell_wide_body.hpp"
#include "bellman.hpp"

namespace aiy {

template <int NP, bool LAB, int NW>
__global__ __launch_bounds__(64 * NW) void bell_wide_kernel(
    BellArgs A, int ntile, int S, int lsb, unsigned long long* __restrict__ old_slots,
    unsigned* __restrict__ cnt, unsigned long long* __restrict__ part, int flags) {
    bell_wide_body<NP, LAB, NW>(A, ntile, S, lsb, old_slots, cnt, part, flags, (int)blockIdx.x);
}

// ------------------------------------------------------------------------------ launcher
template <int NP, bool LAB, int NW>
static int wide_geo(const BellArgs& A, int S, int lsb, unsigned long long* old_slots,
                     unsigned* cnt, unsigned long long* part, int flags, size_t min_lds,
                     hipStream_t st) {
    const int ntile = (A.Na + (1 << lsb) - 1) >> lsb;
    const int items = A.N * ntile;
    const int grid = ((items + 7) / 8) * 8 * S;
    const size_t lds = std::max(bell_wide_lds(A.Na, S, NW), min_lds);
    if (lds > 64 * 1024)  // dynamic LDS past 64 KiB needs the attribute
        AIY_TRY((raise_dynamic_lds<bell_wide_kernel<NP, LAB, NW>>((int)kWideMaxLds)));
    launch_dispatch_timed(bell_wide_kernel<NP, LAB, NW>, dim3(grid), dim3(64 * NW), lds, st, A,
                          ntile, S, lsb, old_slots, cnt, part, flags);
    return AIY_OK;
}
template <int NP, bool LAB>
static int wide_w(const BellArgs& A, int S, int NW, int lsb, unsigned long long* old_slots,
                   unsigned* cnt, unsigned long long* part, int flags, size_t min_lds,
                   hipStream_t st) {
    switch (NW) {
        case 4: return wide_geo<NP, LAB, 4>(A, S, lsb, old_slots, cnt, part, flags, min_lds, st);
        case 8: return wide_geo<NP, LAB, 8>(A, S, lsb, old_slots, cnt, part, flags, min_lds, st);
        default: return wide_geo<NP, LAB, 16>(A, S, lsb, old_slots, cnt, part, flags, min_lds, st);
    }
}

int launch_bell_wide(const BellArgs& A, int S, int NW, int SB, unsigned long long* old_slots,
                     unsigned* cnt, unsigned long long* part, int flags, size_t min_lds,
                     hipStream_t st) {
    if (A.np < 1 || A.np > 8) return fail(AIY_BAD_ARG, "wide sweep needs integer sigma in [2, 9]");
    if (A.C > 1)  // (C candidate rates: launch_bell_wide_batch)
        return fail(AIY_BAD_ARG, "wide sweep: one candidate rate");
    if (S < 1 || S > kWideMaxSplits || (NW != 4 && NW != 8 && NW != 16) ||
        (SB != 8 && SB != 16 && SB != 32 && SB != 64))
        return fail(AIY_BAD_ARG, "wide sweep: S in [1, %d], NW in {4, 8, 16}, SB in {8, ..., 64}",
                    kWideMaxSplits);
    const int lsb = 31 - __builtin_clz((unsigned)SB);
    if (bell_wide_lds(A.Na, S, NW) > kWideMaxLds)
        return fail(AIY_BAD_SHAPE, "wide sweep: the candidate slice does not fit in LDS");
#define AIY_WCASE(n)                                                               \
    case n:                                                                        \
        rc = A.labor ? wide_w<n, true>(A, S, NW, lsb, old_slots, cnt, part, flags, min_lds, st)   \
                     : wide_w<n, false>(A, S, NW, lsb, old_slots, cnt, part, flags, min_lds, st); \
        break;
    int rc = AIY_OK;
    switch (A.np) {
        AIY_WCASE(1) AIY_WCASE(2) AIY_WCASE(3) AIY_WCASE(4) AIY_WCASE(5) AIY_WCASE(6)
        AIY_WCASE(7) AIY_WCASE(8)
    }
#undef AIY_WCASE
    AIY_TRY(rc);
    AIY_HIP(hipGetLastError());
    return AIY_OK;
}

}  // namespace aiy
