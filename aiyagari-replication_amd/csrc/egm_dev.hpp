// Device arithmetic shared by the EGM kernels (egm_kernels.hip, egm_batch_kernels.hip,
// transition_kernels.hip): the marginal utility, the labour first-order condition and interp1 on
// an LDS row, the same operations in every kernel.
#pragma once
#include "aiy_common.hpp"

namespace aiy {

__device__ __forceinline__ double uprime_dev(double c, double sigma, int ns) {
    return ns > 0 ? 1.0 / aiy_ipow(c, ns) : aiy_pow(c, -sigma);  // c.^(-sigma)
}

__device__ __forceinline__ double labor_dev(double c, double ws, double sigma, int ns,
                                            double phi, double theta) {
    double x = (ws * uprime_dev(c, sigma, ns)) / phi;  // u_prime_l_inv(w s .* u_prime_c(c))
    return (1.0 / theta == 1.0) ? x : aiy_pow(x, 1.0 / theta);
}

// interp1(â_j, y_j, q, 'linear', 'extrap') on the LDS row: the count by binary search, the
// segment clamp(count, 1, Na−1) − 1 and the formula of egm_fused_kernel
__device__ __forceinline__ double egm_batch_interp(const double* __restrict__ x,
                                                   const double* __restrict__ y, int Na,
                                                   double q) {
    int lo = 0, hi = Na;  // #{k : â_k <= q}
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    int sgi = lo - 1;
    sgi = sgi < 0 ? 0 : sgi;
    sgi = sgi > Na - 2 ? Na - 2 : sgi;
    const double x0 = x[sgi], x1 = x[sgi + 1];
    const double tt = (q - x0) / (x1 - x0);
    return y[sgi] + tt * (y[sgi + 1] - y[sgi]);
}

}  // namespace aiy
