/* CPU restatement of the labour economy's backward transition pass (TEST INFRASTRUCTURE ONLY).
 *
 * The C oracle's orc_labor_egm_step has one r per step; a transition discounts with next period's
 * rate and budgets with this period's prices.  lref_labor_step2 is orc_labor_egm_step operation
 * for operation with r split into r_next (the Euler sum) and r_now (the rest); lref_labor_backward
 * chains it from the terminal policy, t = T-1 .. 0.  Built with oracle/Makefile's floating-point
 * flags (-O2 -ffp-contract=off -fno-fast-math): every operation rounds as written. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../aiyagari-replication_amd/csrc/aiy_math.h"

static double uprime(double c, double sigma) { return aiy_pow(c, -sigma); }

static double labor_of(double c, double ws, double sigma, double phi, double theta) {
    double x = (ws * uprime(c, sigma)) / phi;
    return (1.0 / theta == 1.0) ? x : aiy_pow(x, 1.0 / theta);
}

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

static double interp_one(int64_t n, const double* x, const double* y, double q) {
    int64_t i = seg_of(n, x, q);
    double t = (q - x[i]) / (x[i + 1] - x[i]);
    return y[i] + t * (y[i + 1] - y[i]);
}

/* One two-rate labour step.  pc_next [N][Na] -> pc_now, pk_now, pl_now [N][Na]; ahat_out
 * (nullable) receives the endogenous grid.  Returns 1 when some row of it is not increasing (NaN
 * included), 0 when all are, -1 when memory runs out. */
int lref_labor_step2(int64_t N, int64_t Na, const double* pc_next, const double* a_grid,
                     const double* s, const double* P, double r_next, double r_now, double w_now,
                     double beta, double sigma, double phi, double theta, double amin,
                     double* pc_now, double* pk_now, double* pl_now, double* ahat_out) {
    double* ah = (double*)malloc(sizeof(double) * (size_t)(N * Na));
    double* cn = (double*)malloc(sizeof(double) * (size_t)(N * Na));
    if (!ah || !cn) {
        free(ah);
        free(cn);
        return -1;
    }
    for (int64_t ja = 0; ja < N * Na; ++ja) {
        int64_t j = ja / Na, a = ja % Na;
        double ws = w_now * s[j];
        double acc = 0.0;
        for (int64_t m = 0; m < N; ++m)
            acc = acc + ((beta * (1 + r_next)) * P[j * N + m]) * uprime(pc_next[m * Na + a], sigma);
        cn[ja] = aiy_pow(acc, -1.0 / sigma);
        double ls = labor_of(cn[ja], ws, sigma, phi, theta);
        ah[ja] = ((cn[ja] + a_grid[a]) - ws * ls) / (1 + r_now);
    }
    int bad = 0;
    for (int64_t ja = 0; ja < N * Na; ++ja) {
        int64_t j = ja / Na, a = ja % Na;
        double ws = w_now * s[j];
        if (a > 0 && !(ah[ja - 1] < ah[ja])) bad = 1;
        double g = interp_one(Na, ah + j * Na, cn + j * Na, a_grid[a]);
        if (a_grid[a] < amin) g = amin;
        pc_now[ja] = g;
        pl_now[ja] = labor_of(g, ws, sigma, phi, theta);
        double k = ((1 + r_now) * a_grid[a] + ws * pl_now[ja]) - g;
        pk_now[ja] = (k < 0) ? 0.0 : k;
    }
    if (ahat_out) memcpy(ahat_out, ah, sizeof(double) * (size_t)(N * Na));
    free(ah);
    free(cn);
    return bad;
}

/* The backward loop: r [T+1], w [T], pc_T [N][Na] -> pk, pl, pc (nullable) [T][N][Na].  A period
 * whose endogenous grid is not increasing stops the loop: *status = 1, *fail_t = that period (its
 * own outputs are written but undefined; the periods below it are left alone). */
int lref_labor_backward(int64_t N, int64_t Na, int64_t T, const double* r, const double* w,
                        const double* pc_T, const double* a_grid, const double* s,
                        const double* P, double beta, double sigma, double phi, double theta,
                        double amin, double* pk, double* pl, double* pc, int32_t* status,
                        int32_t* fail_t) {
    const size_t n = (size_t)(N * Na);
    double* cur = (double*)malloc(sizeof(double) * n);
    double* nxt = (double*)malloc(sizeof(double) * n);
    if (!cur || !nxt) {
        free(cur);
        free(nxt);
        return 1;
    }
    memcpy(cur, pc_T, sizeof(double) * n);
    *status = 0;
    *fail_t = -1;
    for (int64_t t = T - 1; t >= 0; --t) {
        int bad = lref_labor_step2(N, Na, cur, a_grid, s, P, r[t + 1], r[t], w[t], beta, sigma,
                                   phi, theta, amin, nxt, pk + (size_t)t * n, pl + (size_t)t * n,
                                   NULL);
        if (pc) memcpy(pc + (size_t)t * n, nxt, sizeof(double) * n);
        if (bad) {
            *status = bad < 0 ? -1 : 1;
            *fail_t = (int32_t)t;
            break;
        }
        double* tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    free(cur);
    free(nxt);
    return 0;
}
