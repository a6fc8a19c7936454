// A6/A7 batch entry points: the VFI loop of Krusell_Smith_VFI.m:143-204 for C candidate
// economies in one launch, one workgroup each (ks_fused_vfi_batch_kernel).  Layouts are
// candidate-major, as ks_egm_solve_batch: value / k_opt [C] blocks of k x K x 4 column-major,
// K_grid [C][nK], B [C][4], P [C] of MATLAB's 4 x 4, params [C][13].  There is no tiled
// fallback: a size ks_vfi_solve would run tiled is refused with AIY_BAD_SHAPE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "aiy_common.hpp"
#include "host_ctx.hpp"
#include "ks.hpp"

namespace aiy {

// what both tiers check on their host arguments, before any device work
static int check_vfi_batch(int64_t C, int64_t nk, int64_t nK, int64_t howard_steps,
                           int64_t max_vfi) {
    if (C < 1 || C > kVfiBatchMaxCand) return fail(AIY_BAD_SHAPE, "need 1 <= C <= 65,535 candidates");
    if (nk < 3 || nK < 1) return fail(AIY_BAD_SHAPE, "need k_size >= 3 and K_size >= 1");
    if (max_vfi < 1 || max_vfi > 2147483647 || howard_steps < 0 || howard_steps > 2147483647)
        return fail(AIY_BAD_ARG, "max_vfi in [1, 2^31), howard_steps in [0, 2^31)");
    if (nk > 4096 || nK > 4096 || !ks_fused_fits((int)nk, (int)nK))
        return fail(AIY_BAD_SHAPE, "k_size x K_size too large for the one-workgroup VFI solve "
                                   "(the batch has no tiled path; ks_vfi_solve has)");
    return AIY_OK;
}

// device scratch of one call: the candidates' KsVfiCand blocks, then their slice tables
static size_t vfi_batch_scratch(int64_t C, int64_t nK) {
    return (size_t)C * (sizeof(KsVfiCand) + 4 * (size_t)nK * sizeof(KsSlice));
}

// threads per economy: 0 (the library's choice) unless the A/B tool's knob names a geometry
static int vfi_batch_threads_knob() {
    const char* s = getenv("AIY_KS_VFI_BATCH_THREADS");  // (tools/ks_vfi_batch_ab.py)
    return s && *s ? atoi(s) : 0;
}

// Builds the candidates' tables on the host (libm, by ks_slices), uploads them into `scratch`
// and enqueues the one launch.  The upload is ordered on `st` behind whatever still reads
// `scratch`, and the call waits for it before the host tables die; the solve itself is left
// running on `st`.
static int vfi_batch_dev(int64_t C, double* value, double* k_opt, const double* k_grid,
                         const double* K_grid, const double* B, const double* P,
                         const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                         double tol, int64_t max_vfi, int64_t* iters, double* rel_diff,
                         void* scratch, hipStream_t st) {
    std::vector<KsVfiCand> cand(C);
    std::vector<KsSlice> slices((size_t)C * 4 * nK), one;
    for (int64_t c = 0; c < C; ++c) {
        KsParams p;
        memcpy(&p, params + 13 * c, sizeof p);
        ks_slices(p, B + 4 * c, K_grid + c * nK, (int)nK, one);
        std::copy(one.begin(), one.end(), slices.begin() + (size_t)c * 4 * nK);
        p_rows(P + 16 * c, cand[c].P);
        cand[c].beta = p.beta;
        cand[c].k_min = p.k_min;
        cand[c].k_max = p.k_max;
    }
    KsVfiCand* dcand = (KsVfiCand*)scratch;
    KsSlice* dsl = (KsSlice*)(dcand + C);
    AIY_HIP(hipMemcpyAsync(dcand, cand.data(), cand.size() * sizeof(KsVfiCand),
                           hipMemcpyHostToDevice, st));
    AIY_HIP(hipMemcpyAsync(dsl, slices.data(), slices.size() * sizeof(KsSlice),
                           hipMemcpyHostToDevice, st));
    AIY_HIP(hipStreamSynchronize(st));
    KsVfiBatchArgs A{};
    A.nk = (int)nk;
    A.nK = (int)nK;
    A.howard = (int)howard_steps;
    A.max_vfi = (int)max_vfi;
    A.C = (int)C;
    A.k_grid = k_grid;
    A.cand = dcand;
    A.slice = dsl;
    A.tol = tol;
    A.value = value;
    A.k_opt = k_opt;
    A.iters = iters;
    A.rel = rel_diff;
    return launch_ks_fused_batch(A, vfi_batch_threads_knob(), st);
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int64_t ks_vfi_batch_scratch_bytes(int64_t C, int64_t nK) {
    return (C < 1 || nK < 1) ? 0 : (int64_t)vfi_batch_scratch(C, nK);
}

int ks_vfi_solve_batch_dev(int64_t C, double* value, double* k_opt, const double* k_grid,
                           const double* K_grid, const double* B, const double* P,
                           const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                           double tol, int64_t max_vfi, int64_t* iters, double* rel_diff,
                           void* scratch, void* stream) {
    if (!value || !k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !rel_diff ||
        !scratch)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_vfi_batch(C, nk, nK, howard_steps, max_vfi));
    return vfi_batch_dev(C, value, k_opt, k_grid, K_grid, B, P, params, nk, nK, howard_steps, tol,
                         max_vfi, iters, rel_diff, scratch, (hipStream_t)stream);
}

int ks_vfi_solve_batch(int64_t C, double* value, double* k_opt, const double* k_grid,
                       const double* K_grid, const double* B, const double* P,
                       const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                       double tol, int64_t max_vfi, int64_t* iters, double* rel_diff) {
    if (!value || !k_opt || !k_grid || !K_grid || !B || !P || !params || !iters || !rel_diff)
        return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_vfi_batch(C, nk, nK, howard_steps, max_vfi));
    AIY_TRY(check_grid_strict(k_grid, nk));  // pchip divides by k(i+1) - k(i)
    const size_t n1 = (size_t)nk * nK * 4, n = (size_t)C * n1;
    for (int64_t c = 0; c < C; ++c)  // ±inf refused as in ks_vfi_solve (ks_check_value); NaN passes
        for (size_t q = 0; q < n1; ++q)
            if (std::isinf(value[c * n1 + q]))
                return fail(AIY_NON_FINITE,
                            "value(%lld) of candidate %lld is infinite (finite or NaN entries only)",
                            (long long)q + 1, (long long)c + 1);
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(4 * nK, nk, 1, &c));
    double *dkg, *dV, *dk, *drel;
    int64_t* dit;
    unsigned char* dscr;
    AIY_TRY(c->up("vfib_kg", k_grid, nk, &dkg));
    AIY_TRY(c->up("vfib_V", value, n, &dV));
    AIY_TRY(c->up("vfib_k", k_opt, n, &dk));
    AIY_TRY(c->room("vfib_iters", C, &dit));
    AIY_TRY(c->room("vfib_rel", C, &drel));
    AIY_TRY(c->room("vfib_scratch", vfi_batch_scratch(C, nK), &dscr));
    AIY_TRY(vfi_batch_dev(C, dV, dk, dkg, K_grid, B, P, params, nk, nK, howard_steps, tol, max_vfi,
                          dit, drel, dscr, c->st));
    AIY_TRY(c->down(iters, dit, C));
    AIY_TRY(c->down(rel_diff, drel, C));
    AIY_TRY(c->down(value, dV, n));
    AIY_TRY(c->down(k_opt, dk, n));
    AIY_HIP(hipStreamSynchronize(c->st));
    return AIY_OK;
}

}  // extern "C"
