// Stand-alone host program around the host tier's name -> buffer map and its typed staging
// (csrc/host_ctx.hpp: NamedBufs, Staging; tests/test_host_layer_cpu.py builds it with
// -fsanitize=address,undefined).  Both are driven through a malloc-backed memory whose copies are
// memcpy, so the sanitizer sees every leak, double free and access past a buffer's or a staging
// vector's extent.  No device is needed and none is touched.
// Prints one "ok" line per property; exits nonzero at the first one that does not hold.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "host_ctx.hpp"

namespace aiy {
int fail(int code, const char*, ...) { return code; }
}  // namespace aiy

static bool g_oom = false;
static int g_live = 0;
struct HostMem {
    static hipError_t alloc(void** p, size_t bytes) {
        if (g_oom) return hipErrorOutOfMemory;
        *p = malloc(bytes);
        ++g_live;
        return hipSuccess;
    }
    static void free(void* p) {
        ::free(p);
        --g_live;
    }
};

#define CHECK(cond)                                           \
    do {                                                      \
        if (!(cond)) {                                        \
            printf("FAILED %s (line %d)\n", #cond, __LINE__); \
            return 1;                                         \
        }                                                     \
        printf("ok %s\n", #cond);                             \
    } while (0)

static int named_bufs() {
    {
        aiy::NamedBufs<HostMem> B;
        void *a = nullptr, *a2 = nullptr, *b = nullptr, *z = nullptr;
        CHECK(B.get("a", 100, &a) == AIY_OK && a && g_live == 1 && B.bytes() == 100);
        memset(a, 1, 100);  // (the sanitizer checks the extent)
        CHECK(B.get("a", 40, &a2) == AIY_OK && a2 == a && g_live == 1 && B.bytes() == 100);
        CHECK(B.get("a", 100, &a2) == AIY_OK && a2 == a);
        CHECK(B.get("b", 100, &b) == AIY_OK && b && b != a && g_live == 2);  // two names
        memset(b, 2, 100);
        CHECK(((unsigned char*)a)[99] == 1);
        CHECK(B.get("a", 101, &a2) == AIY_OK && a2 && g_live == 2 && B.bytes() == 201);
        memset(a2, 3, 101);  // a larger request replaced it: exactly what was asked
        CHECK(((unsigned char*)b)[0] == 2 && ((unsigned char*)b)[99] == 2);
        CHECK(B.get("z", 0, &z) == AIY_OK && z && z != a2 && z != b && g_live == 3);
        g_oom = true;
        void* f = &g_oom;
        CHECK(B.get("b", 1000, &f) == AIY_NO_MEMORY && f == nullptr && g_live == 2);
        CHECK(B.get("new", 8, &f) == AIY_NO_MEMORY && f == nullptr && g_live == 2);
        g_oom = false;
        CHECK(B.get("b", 1000, &f) == AIY_OK && f && g_live == 3);  // reusable after a failure
        memset(f, 4, 1000);
    }  // destruction frees every buffer (and the sanitizer's leak check agrees)
    CHECK(g_live == 0);
    return 0;
}

// the staging's device on the same memory: a copy is a memcpy (done when the call returns), the
// wait counts its calls
static int g_syncs = 0;
struct HostDev : HostMem {
    static hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
        memcpy(dst, src, bytes);
        return hipSuccess;
    }
    static hipError_t sync(hipStream_t) {
        ++g_syncs;
        return hipSuccess;
    }
};

static int staging() {
    {
        aiy::Staging<HostDev> S;
        // bcast: C blocks, every one the host block; exactly n * C elements (the sanitizer checks)
        const double blk[3] = {1.5, -2.5, 3.5};
        double* b = nullptr;
        CHECK(S.bcast("b", blk, 3, 4, &b) == AIY_OK && b && g_live == 1);
        CHECK(S.bufs.bytes() == 3 * 4 * sizeof(double));
        bool same = true;
        for (int q = 0; q < 4; ++q) same = same && memcmp(b + 3 * q, blk, sizeof blk) == 0;
        CHECK(same);
        double* b1 = nullptr;
        CHECK(S.bcast("b", blk, 3, 1, &b1) == AIY_OK && b1 == b);  // C = 1: the upload alone
        // up_rows: two 2 x 3 column-major arrays as [2][2][3] rows, from storage of its own
        const int N = 2, Na = 3;
        double cm[12];
        for (int k = 0; k < 12; ++k) cm[k] = 10.0 * (k / 6) + (k % 6);  // cm(i, j) = i + 2 j
        double* r = nullptr;
        CHECK(S.up_rows("r", cm, N, Na, 2, &r) == AIY_OK && r && S.held.size() == 1);
        bool rows = true;
        for (int q = 0; q < 2; ++q)
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < Na; ++j)
                    rows = rows && r[q * 6 + i * Na + j] == 10.0 * q + (i + N * j);
        CHECK(rows);
        // every upload in flight keeps its own source: a second one does not touch the first's
        double* r2 = nullptr;
        CHECK(S.up_rows("r2", cm + 6, N, Na, 1, &r2) == AIY_OK && S.held.size() == 2);
        CHECK(S.held[0] != S.held[1] && r[0] == 0.0 && r2[0] == 10.0);
        // up_own: a vector handed over, int elements
        int* iv = nullptr;
        std::vector<int> three = {4, 5, 6};
        CHECK(S.up_own("i", std::move(three), &iv) == AIY_OK && iv[2] == 6);
        CHECK(S.held.size() == 3 && g_syncs == 0);
        // down_rows: the twin; it waits once and lets go of the sources
        double back[12];
        memset(back, 0xff, sizeof back);
        CHECK(S.down_rows(back, r, N, Na, 2) == AIY_OK && memcmp(back, cm, sizeof cm) == 0);
        CHECK(g_syncs == 1 && S.held.empty());
        int ib[3] = {0, 0, 0};
        CHECK(S.down(ib, iv, 3) == AIY_OK && ib[0] == 4 && ib[2] == 6 && g_syncs == 1);
        CHECK(S.sync() == AIY_OK && g_syncs == 2);
        // allocation failure: the status comes back, nothing is copied, the source is let go of
        // at the next wait
        g_oom = true;
        double* f = b;
        CHECK(S.bcast("big", blk, 3, 1000, &f) == AIY_NO_MEMORY && f == nullptr);
        CHECK(S.up_rows("big", cm, N, Na, 2, &f) == AIY_NO_MEMORY && f == nullptr);
        g_oom = false;
        CHECK(S.sync() == AIY_OK && S.held.empty());
    }
    CHECK(g_live == 0);
    return 0;
}

int main() {
    if (named_bufs()) return 1;
    if (staging()) return 1;
    printf("done\n");
    return 0;
}
