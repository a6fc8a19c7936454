// Device helpers shared by the histogram kernels (dist_kernels.hip, dist_batch_kernels.hip): a
// destination's mass from its run(s) of sources, in the A10 order dist.hpp defines.
#pragma once
#include "aiy_common.hpp"
#include "dist.hpp"

namespace aiy {

// term of source j for a destination whose lottery run of the node below ends at js; the
// source arrays are indexed from `base` (0 for the global rows, the wave's first source for
// its LDS copy)
template <bool LOT>
__device__ __forceinline__ double dist_term(const double* __restrict__ lam,
                                            const double* __restrict__ wr, int j, int js,
                                            int base) {
    if (!LOT) return lam[j - base];
    const double w = wr[j - base];
    return j < js ? lam[j - base] * w : lam[j - base] * (1 - w);
}

// sequential sum of the terms of sources [b, e) (e − b ≤ kDistChunk), 8 loads in flight
template <bool LOT>
__device__ __forceinline__ double dist_chunk(const double* __restrict__ lam,
                                             const double* __restrict__ wr, int b, int e,
                                             int js, int base) {
    double part = 0.0;
    for (int t0 = b; __ballot(t0 < e) != 0ull; t0 += 8) {  // wave-uniform trip count
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            x[u] = (t0 + u < e) ? dist_term<LOT>(lam, wr, t0 + u, js, base) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < e) part = part + x[u];
    }
    return part;
}

// a destination's mass from its run(s) [jb, je) in the A10 order: short runs by the lane's own
// sequential sum (== the chunked sum for L <= G); long runs one at a time, lane c summing
// chunks c, c + 64, ... and the chunk sums folded in chunk order with wave-uniform reads
template <bool LOT>
__device__ __forceinline__ double dist_mass(const double* __restrict__ lam,
                                            const double* __restrict__ wr, int jb, int js,
                                            int je, int base) {
    const int lane = threadIdx.x & 63;
    const int L = je - jb;
    constexpr int G = kDistChunk;
    double tot = dist_chunk<LOT>(lam, wr, jb, L <= G ? je : jb, js, base);
    unsigned long long lm = __ballot(L > G);
    while (lm) {
        const int q = __builtin_ctzll(lm);
        lm &= lm - 1;
        const int qb = readlane_i(jb, q), qs = readlane_i(js, q), qL = readlane_i(L, q);
        const int nch = (qL + G - 1) / G;
        double total = 0.0;
        for (int c0 = 0; c0 < nch; c0 += 64) {
            const int c = c0 + lane;
            const int b = qb + c * G;
            const int e = c < nch ? min(b + G, qb + qL) : b;
            const double part = dist_chunk<LOT>(lam, wr, b, e, qs, base);
            const int nc = min(64, nch - c0);
            for (int u = 0; u < nc; ++u) total = total + readlane_d(part, u);
        }
        if (lane == q) tot = total;
    }
    return tot;
}

}  // namespace aiy
