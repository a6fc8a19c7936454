// Device arithmetic shared by the EGM kernels (egm_kernels.hip, egm_batch_kernels.hip): the
// marginal utility and the labour first-order condition, the same operations in every kernel.
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

}  // namespace aiy
