/* CPU restatement of the expectation vectors of the sequence-space Jacobian (TEST INFRASTRUCTURE
 * ONLY): dist_expect_batch_kernel operation for operation.  The plan is dist_keys_kernel's — the
 * clamp, the bracket, the weight wr of the upper node — and wl = 1 - wr the lower node's; then
 *   G_t(i,k') = sum_m P(i,m) E_t(m,k')  (m ascending, from +0),
 *   E_{t+1}(i,k) = wl(i,k) G_t(i,lo(i,k)) + (1 - wl(i,k)) G_t(i,lo(i,k)+1).
 * Built with oracle/Makefile's floating-point flags (-O2 -ffp-contract=off -fno-fast-math): every
 * operation rounds as written. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int64_t seg_of(int64_t n, const double* x, double q) {
    /* largest i with x[i] <= q, clamped to [0, n-2] */
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (x[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    int64_t i = lo - 1;
    if (i < 0) i = 0;
    if (i > n - 2) i = n - 2;
    return i;
}

/* policy, y0 [N][Na], P row-major [N][N] -> E [T][N][Na]; lo_out (int64) and wl_out [N][Na] are
 * nullable.  Returns 0, or 1 when memory runs out. */
int sref_expect(int64_t N, int64_t Na, int64_t T, const double* policy, const double* y0,
                const double* a, const double* P, double* E, int64_t* lo_out, double* wl_out) {
    const size_t n = (size_t)(N * Na);
    int64_t* lo = (int64_t*)malloc(sizeof(int64_t) * n);
    double* wl = (double*)malloc(sizeof(double) * n);
    double* G = (double*)malloc(sizeof(double) * n);
    if (!lo || !wl || !G) {
        free(lo);
        free(wl);
        free(G);
        return 1;
    }
    const double a0 = a[0], an = a[Na - 1];
    for (size_t e = 0; e < n; ++e) {
        double x = policy[e];
        x = x < a0 ? a0 : x;
        x = x > an ? an : x;
        int64_t key = seg_of(Na, a, x);
        double wr = (x - a[key]) / (a[key + 1] - a[key]);
        wl[e] = 1 - wr;
        lo[e] = key;
    }
    memcpy(E, y0, sizeof(double) * n);
    for (int64_t t = 0; t + 1 < T; ++t) {
        const double* Et = E + (size_t)t * n;
        double* En = E + (size_t)(t + 1) * n;
        for (int64_t i = 0; i < N; ++i)
            for (int64_t k = 0; k < Na; ++k) {
                double acc = 0.0;
                for (int64_t m = 0; m < N; ++m) acc = acc + P[i * N + m] * Et[m * Na + k];
                G[i * Na + k] = acc;
            }
        for (int64_t i = 0; i < N; ++i)
            for (int64_t k = 0; k < Na; ++k) {
                const size_t e = (size_t)(i * Na + k);
                const double* row = G + i * Na;
                En[e] = wl[e] * row[lo[e]] + (1 - wl[e]) * row[lo[e] + 1];
            }
    }
    if (lo_out) memcpy(lo_out, lo, sizeof(int64_t) * n);
    if (wl_out) memcpy(wl_out, wl, sizeof(double) * n);
    free(lo);
    free(wl);
    free(G);
    return 0;
}
