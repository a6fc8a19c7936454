// Launch interface of the dense solve (dense_kernels.hip): C systems A_c·X_c = B_c by Gaussian
// elimination with partial pivoting, one workgroup per system.  All arrays are row-major; arrays
// [C][...] hold block c at c · (the block's size).  A and B are not modified: the kernel works on
// the augmented copy W_c = (A_c | B_c), [n][n+R], in workspace memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aiy {

// Every operation is rounded as written (no fused multiply-add); the operations on one element
// and their order depend on (n, R) and the system's own numbers alone — not on C, the system's
// place in the batch, the block size or the thread that does them.
//
//  1. j = 0 … n−1:
//     pivot: p = j, best = |A[j][j]|; i = j+1 … n−1 ascending: |A[i][j]| > best takes it (ties go
//       to the lowest index; a NaN is never taken over a number).
//     !(best > 0) or best not finite: status 1, fail j, the whole X block NaN, stop.
//     swap rows j and p of A and of B;
//     i > j: l_i = A[i][j]/A[j][j]; A[i][k] = A[i][k] − (l_i·A[j][k]), k > j, and
//       B[i][q] = B[i][q] − (l_i·B[j][q]).
//  2. j = n−1 … 0: X[j][q] = B[j][q]/A[j][j]; B[i][q] = B[i][q] − (A[i][j]·X[j][q]), i < j.
//  3. status 0, fail −1.
struct DenseSolveArgs {
    int C, n, R;
    const double* A;  // device [C][n][n]
    const double* B;  // device [C][n][R]
    double* X;        // device [C][n][R]
    double* W;        // device [C][n][n+R] (workspace)
    int* status;      // device [C]
    int* fail;        // device [C]
};
constexpr int kDenseMaxN = 4096;  // the multipliers of a column sit in LDS (32 KiB)
// the limits every entry states: 1 <= n <= 4096, R >= 1, n·(n + R) < 2^31 (a system's indices are
// ints), C >= 1
inline bool dense_fits(int64_t n, int64_t R) {
    return n >= 1 && n <= kDenseMaxN && R >= 1 && R < (1ll << 31) && n * (n + R) < (1ll << 31);
}
inline size_t dense_work_doubles(int64_t n, int64_t R) { return (size_t)n * (size_t)(n + R); }
int launch_dense_solve_batch(const DenseSolveArgs& A, hipStream_t st);

}  // namespace aiy
