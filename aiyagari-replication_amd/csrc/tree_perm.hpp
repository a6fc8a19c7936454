// Dispatch order of the one-wave-per-tile A1 tree launch (variant bits 6 / 11 / 26), as pure
// host functions of the tiles' costs.  A launch of N·ntile one-wave items on 1,024 SIMDs puts
// three waves on some SIMDs — the last-dispatched items of each XCD — and those items end the
// launch (tools/tree_trace.py: every last-to-finish item sits on a 3-wave SIMD).  The orders keep
// each XCD's contiguous item range (xcd_remap: the same L2 sets) and make the third waves the
// cheapest tiles.  Work order only.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <vector>

namespace aiy {

constexpr int kSimdsPerXcd = 128;  // MI355X: 32 CUs x 4 SIMDs per XCD

// cost of item it = i·ntile + t: the feasible prefixes of the tile's last state, summed over
// the labour levels (the bound tree's superblock count); kl is [Nl][N][ntile]
struct TreeTileCost {
    const std::vector<int>& kl;
    int N, ntile, Nl;
    long long operator()(int it) const {
        const int i = it / ntile, t = it % ntile;
        long long c = 0;
        for (int l = 0; l < Nl; ++l) c += kl[((size_t)l * N + i) * ntile + t];
        return c;
    }
};

// `items` in their own order, but the cheapest size − 2·kSimdsPerXcd of them moved to the end,
// the cheapest at the very end (G: one more than the largest item)
inline std::vector<int> tree_cheapest_last(const std::vector<int>& items, const TreeTileCost& cost,
                                           int G) {
    const int size = (int)items.size(), tail = std::max(0, size - 2 * kSimdsPerXcd);
    std::vector<int> by(items);
    std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return cost(a) < cost(b); });
    std::vector<char> last(G, 0);
    for (int u = 0; u < tail; ++u) last[by[u]] = 1;
    std::vector<int> out;
    for (int it : items)
        if (!last[it]) out.push_back(it);
    for (int u = tail - 1; u >= 0; --u) out.push_back(by[u]);
    return out;
}

// PK one-wave tiles per workgroup (bell_tree_pack); workgroup b runs on XCD b mod 8, its waves
// take slots b·PK .. b·PK + PK − 1; the last workgroup's unused slots hold −1.  Each XCD's range
// is dealt heaviest first (bit 6), or row-major with its cheapest tiles last (bit 11).
inline std::vector<int> tree_perm_order(const std::vector<int>& kl, int N, int ntile, int Nl,
                                        int PK, bool heaviest_first) {
    const TreeTileCost cost{kl, N, ntile, Nl};
    const int G = N * ntile, nwg = (G + PK - 1) / PK, slots = nwg * PK;
    std::vector<int> perm(slots, -1);
    int start = 0;
    for (int x = 0; x < 8; ++x) {
        int size = (nwg / 8 + (x < nwg % 8 ? 1 : 0)) * PK;
        if (x == (nwg - 1) % 8) size -= slots - G;
        std::vector<int> items(size);
        for (int u = 0; u < size; ++u) items[u] = start + u;
        if (heaviest_first)
            std::stable_sort(items.begin(), items.end(),
                             [&](int a, int b) { return cost(a) > cost(b); });
        else
            items = tree_cheapest_last(items, cost, G);
        for (int u = 0; u < size; ++u)  // the XCD's (u / PK)-th workgroup b = 8(u / PK) + x
            perm[(size_t)(8 * (u / PK) + x) * PK + u % PK] = items[u];
        start += size;
    }
    return perm;
}

// The hybrid launch's order (variant bit 26): each XCD keeps its contiguous row-major range; its
// `coop` heaviest tiles become cooperative workgroups (slots {item, −2}), dealt first, heaviest
// first; the rest are packed two per workgroup in row-major order with the range's cheapest
// tiles last ({item, −1} when one is left over).  Workgroup b = 8q + x is XCD x's q-th; XCDs
// with fewer workgroups get empty ({−1, −1}) ones so that b mod 8 still names the XCD.
inline std::vector<int> tree_perm_hybrid_order(const std::vector<int>& kl, int N, int ntile,
                                               int Nl, int coop) {
    const TreeTileCost cost{kl, N, ntile, Nl};
    const int G = N * ntile;
    std::vector<std::array<int, 2>> wg[8];  // per XCD: its workgroups' slot pairs, in order
    int start = 0;
    for (int x = 0; x < 8; ++x) {
        const int size = G / 8 + (x < G % 8 ? 1 : 0);
        std::vector<int> items(size);
        for (int u = 0; u < size; ++u) items[u] = start + u;
        start += size;
        std::vector<int> by(items);
        std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return cost(a) > cost(b); });
        const int H = std::min(size, coop);
        std::vector<char> is_coop(G, 0);
        for (int u = 0; u < H; ++u) {
            is_coop[by[u]] = 1;
            wg[x].push_back({by[u], -2});
        }
        std::vector<int> rest;
        for (int it : items)
            if (!is_coop[it]) rest.push_back(it);
        const std::vector<int> out = tree_cheapest_last(rest, cost, G);
        for (size_t u = 0; u < out.size(); u += 2)
            wg[x].push_back({out[u], u + 1 < out.size() ? out[u + 1] : -1});
    }
    size_t nq = 0;
    for (int x = 0; x < 8; ++x) nq = std::max(nq, wg[x].size());
    std::vector<int> perm(8 * nq * 2, -1);
    for (size_t q = 0; q < nq; ++q)
        for (int x = 0; x < 8; ++x)
            if (q < wg[x].size()) {
                perm[(8 * q + x) * 2] = wg[x][q][0];
                perm[(8 * q + x) * 2 + 1] = wg[x][q][1];
            }
    return perm;
}

}  // namespace aiy
