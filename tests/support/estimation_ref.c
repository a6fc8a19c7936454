/* CPU restatement of the autocovariances and the Gaussian log-likelihood of one candidate (TEST
 * INFRASTRUCTURE ONLY): ssj_loglik_batch_kernel operation for operation, as csrc/lik.hpp writes
 * the arithmetic out.  n = L n_o, row i = t n_o + o:
 *   1. Gamma[l][o][p] = sum_{u=0}^{T-1-l} m[o][u+l] m[p][u], u ascending from +0 (l >= T: +0);
 *   2. V[i][k] (k <= i) = Gamma[t-t'][o][p], the diagonal Gamma[0][o][o] + me_var[o]; z = y;
 *   3. j ascending: d_j = V[j][j]; !(d_j > 0): status 1, fail j, loglik NaN, d[j+1..] NaN; else
 *      w_i = V[i][j], l_i = w_i / d_j, V[i][k] = V[i][k] - (l_i w_k) for j < k <= i, and the same
 *      for z as row n (w_n = z_j);
 *   4. logdet = sum_j aiy_log(d_j), quad = sum_j (z_j z_j) / d_j, j ascending from +0;
 *      loglik = -0.5 ((n 1.8378770664093453 + logdet) + quad).
 * Built with oracle/Makefile's floating-point flags (-O2 -ffp-contract=off -fno-fast-math): every
 * operation rounds as written. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../aiyagari-replication_amd/csrc/aiy_math.h"

/* m [n_o][T], y [L][n_o] (nullable: Gamma only), me_var [n_o]; Gamma [L][n_o][n_o] and d [n] are
 * nullable.  Returns 0, or 2 when memory runs out; the candidate's status goes to *status. */
int eref_loglik(int64_t n_o, int64_t T, int64_t L, const double* m, const double* y,
                const double* me_var, double* loglik, int32_t* status, int32_t* fail_j,
                double* Gamma, double* d) {
    const int64_t n = n_o * L;
    double* G = (double*)malloc(sizeof(double) * (size_t)(n * n_o));
    if (!G) return 2;
    for (int64_t l = 0; l < L; ++l)
        for (int64_t o = 0; o < n_o; ++o)
            for (int64_t p = 0; p < n_o; ++p) {
                double acc = 0.0;
                for (int64_t u = 0; u < T - l; ++u) acc = acc + m[o * T + u + l] * m[p * T + u];
                G[(l * n_o + o) * n_o + p] = acc;
            }
    if (Gamma)
        for (int64_t e = 0; e < n * n_o; ++e) Gamma[e] = G[e];
    if (!y) {
        free(G);
        return 0;
    }
    double* V = (double*)malloc(sizeof(double) * (size_t)(n * (n + 1) / 2));
    double* w = (double*)malloc(sizeof(double) * (size_t)(n + 1));
    double* li = (double*)malloc(sizeof(double) * (size_t)(n + 1));
    double* z = (double*)malloc(sizeof(double) * (size_t)n);
    if (!V || !w || !li || !z) {
        free(G);
        free(V);
        free(w);
        free(li);
        free(z);
        return 2;
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k <= i; ++k) {
            const int64_t t = i / n_o, o = i % n_o, tp = k / n_o, p = k % n_o;
            double v = G[((t - tp) * n_o + o) * n_o + p];
            if (i == k) v = v + me_var[o];
            V[i * (i + 1) / 2 + k] = v;
        }
    for (int64_t k = 0; k < n; ++k) z[k] = y[k];
    int64_t failed = -1;
    for (int64_t j = 0; j < n; ++j) {
        const double dj = V[j * (j + 1) / 2 + j];
        if (!(dj > 0)) {
            failed = j;
            break;
        }
        for (int64_t i = j + 1; i <= n; ++i) {
            w[i] = i < n ? V[i * (i + 1) / 2 + j] : z[j];
            li[i] = w[i] / dj;
        }
        for (int64_t i = j + 1; i < n; ++i)
            for (int64_t k = j + 1; k <= i; ++k)
                V[i * (i + 1) / 2 + k] = V[i * (i + 1) / 2 + k] - li[i] * w[k];
        for (int64_t k = j + 1; k < n; ++k) z[k] = z[k] - li[n] * w[k];
    }
    if (failed >= 0) {
        if (d)
            for (int64_t k = 0; k < n; ++k) d[k] = k <= failed ? V[k * (k + 1) / 2 + k] : NAN;
        *loglik = NAN;
        *status = 1;
        *fail_j = (int32_t)failed;
    } else {
        double logdet = 0.0, quad = 0.0;
        for (int64_t k = 0; k < n; ++k) {
            const double dk = V[k * (k + 1) / 2 + k];
            logdet = logdet + aiy_log(dk);
            if (d) d[k] = dk;
        }
        for (int64_t k = 0; k < n; ++k) quad = quad + (z[k] * z[k]) / V[k * (k + 1) / 2 + k];
        *loglik = -0.5 * (((double)n * 1.8378770664093453 + logdet) + quad);
        *status = 0;
        *fail_j = -1;
    }
    free(G);
    free(V);
    free(w);
    free(li);
    free(z);
    return 0;
}
