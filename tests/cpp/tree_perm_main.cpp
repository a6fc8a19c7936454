// Stand-alone host program around csrc/tree_perm.hpp (tests/test_host_layer_cpu.py builds it with
// -fsanitize=address,undefined).  stdin: the number of cases, then per case
//   N ntile Nl PK mode coop   (mode 0: heaviest first, 1: cheapest last, 2: hybrid)
// followed by the Nl·N·ntile entries of kl.  stdout: one line per case, the slot vector.
#include <cstdio>
#include <vector>

#include "tree_perm.hpp"

int main() {
    int ncase = 0;
    if (scanf("%d", &ncase) != 1) return 2;
    for (int c = 0; c < ncase; ++c) {
        int N, ntile, Nl, PK, mode, coop;
        if (scanf("%d %d %d %d %d %d", &N, &ntile, &Nl, &PK, &mode, &coop) != 6) return 2;
        std::vector<int> kl((size_t)Nl * N * ntile);
        for (int& v : kl)
            if (scanf("%d", &v) != 1) return 2;
        const std::vector<int> perm = mode == 2
                                          ? aiy::tree_perm_hybrid_order(kl, N, ntile, Nl, coop)
                                          : aiy::tree_perm_order(kl, N, ntile, Nl, PK, mode == 0);
        for (size_t u = 0; u < perm.size(); ++u) printf(u ? " %d" : "%d", perm[u]);
        printf("\n");
    }
    return 0;
}
