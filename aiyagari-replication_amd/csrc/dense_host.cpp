// Dense solve entry points: C systems A_c·X_c = B_c, one workgroup each (aiy_dense_solve_batch
// [_dev]; dense.hpp states the arithmetic operation for operation).  Everything a host entry can
// refuse it refuses before it asks for a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "aiy_common.hpp"
#include "dense.hpp"
#include "host_ctx.hpp"

namespace aiy {

static int check_dense(int64_t C, int64_t n, int64_t R) {
    if (C < 1 || C > (1ll << 31) - 1) return fail(AIY_BAD_SHAPE, "need 1 <= C < 2^31");
    if (n < 1 || n > kDenseMaxN) return fail(AIY_BAD_SHAPE, "need 1 <= n <= 4096");
    if (R < 1) return fail(AIY_BAD_SHAPE, "need R >= 1");
    if (!dense_fits(n, R)) return fail(AIY_BAD_SHAPE, "need n·(n + R) < 2^31");
    return AIY_OK;
}

static int dense_dev(int64_t C, int64_t n, int64_t R, const double* A, const double* B, double* X,
                     double* W, int* status, int* fail_j, hipStream_t st) {
    DenseSolveArgs D{};
    D.C = (int)C; D.n = (int)n; D.R = (int)R;
    D.A = A; D.B = B; D.X = X; D.W = W; D.status = status; D.fail = fail_j;
    return launch_dense_solve_batch(D, st);
}

}  // namespace aiy

using namespace aiy;

extern "C" {

int aiy_dense_solve_batch_dev(int64_t C, int64_t n, int64_t R, const double* A, const double* B,
                              double* X, double* work, int32_t* status, int32_t* fail_j,
                              void* stream) {
    if (!A || !B || !X || !work || !status || !fail_j) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_dense(C, n, R));
    return dense_dev(C, n, R, A, B, X, work, status, fail_j, (hipStream_t)stream);
}

int aiy_dense_solve_batch(int64_t C, int64_t n, int64_t R, const double* A, const double* B,
                          double* X, int32_t* status, int32_t* fail_j, int64_t chunk) {
    if (!A || !B || !X || !status || !fail_j) return fail(AIY_BAD_ARG, "NULL argument");
    AIY_TRY(check_dense(C, n, R));
    if (chunk < 0) return fail(AIY_BAD_ARG, "chunk must be >= 0 (0: the default)");
    const size_t nn = (size_t)n * n, nr = (size_t)n * R;
    if (chunk == 0) {  // A, B, X and the working copy of a system
        const size_t per = sizeof(double) * 2 * (nn + nr) + 2 * sizeof(int);
        chunk = (int64_t)std::max<size_t>(1, kBatchStageBytes / per);
    }
    chunk = std::min(chunk, C);
    std::lock_guard<std::mutex> lk(host_mutex());
    HostCtx* c;
    AIY_TRY(get_ctx(1, 2, 1, &c));
    for (int64_t c0 = 0; c0 < C; c0 += chunk) {
        const size_t m = (size_t)std::min(chunk, C - c0);
        double *dA, *dB, *dX, *dW;
        int *dst, *dfl;
        AIY_TRY(c->up("dense_A", A + (size_t)c0 * nn, m * nn, &dA));
        AIY_TRY(c->up("dense_B", B + (size_t)c0 * nr, m * nr, &dB));
        AIY_TRY(c->room("dense_X", m * nr, &dX));
        AIY_TRY(c->room("dense_W", m * (nn + nr), &dW));
        AIY_TRY(c->room("dense_st", m, &dst));
        AIY_TRY(c->room("dense_fl", m, &dfl));
        AIY_TRY(dense_dev((int64_t)m, n, R, dA, dB, dX, dW, dst, dfl, c->st));
        AIY_TRY(c->down(X + (size_t)c0 * nr, dX, m * nr));
        AIY_TRY(c->down(status + c0, dst, m));
        AIY_TRY(c->down(fail_j + c0, dfl, m));
        AIY_TRY(c->sync());  // the next chunk reuses the buffers
    }
    return AIY_OK;
}

}  // extern "C"
