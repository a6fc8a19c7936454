// Stand-alone host program around the batched histogram solve's blocks (DistBatchBlocksT,
// csrc/devbuf.hpp) and its fit rule (csrc/dist.hpp), built with -fsanitize=address,undefined by
// tests/test_dist_batch_cpu.py and run with no device visible.  The group is driven through a
// malloc-backed memory that can be told to fail at the k-th allocation, so the sanitizer sees
// every leak, double free and write past a block sized for C candidates of n states; the real
// group is checked where every allocation fails.
// Prints one "ok" line per property; exits nonzero at the first one that does not hold.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "devbuf.hpp"
#include "dist.hpp"

static std::string g_err;
namespace aiy {
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace aiy

static int g_fail_at = -1;  // the allocation (counted from 0) that fails; -1: none
static int g_allocs = 0, g_live = 0;
struct HostMem {
    static hipError_t alloc(void** p, size_t bytes) {
        if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
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

using Blocks = aiy::DistBatchBlocksT<HostMem, HostMem>;
constexpr int kBufs = 10;  // allocations of one group

// what aiy_dist_stationary_batch_dev and its kernels do with blocks sized for C candidates of
// n states and nw offsets: every element written
static void touch(Blocks& b, size_t C, size_t n, size_t nw) {
    for (size_t q = 0; q < C * n; ++q) {
        b.key.get()[q] = (int)q;
        b.wr.get()[q] = 0.5;
    }
    for (size_t q = 0; q < C * nw; ++q) b.off.get()[q] = (int)q;
    for (size_t q = 0; q < C * 256; ++q) b.part.get()[q] = 1.0;
    for (size_t c = 0; c < C; ++c) {
        b.hflags.get()[c] = 0u;
        b.hiters.get()[c] = (long long)c;
        b.hdist.get()[c] = 0.5;
    }
    memcpy(b.flags.get(), b.hflags.get(), sizeof(unsigned) * C);
    memcpy(b.iters.get(), b.hiters.get(), sizeof(long long) * C);
    memcpy(b.dist.get(), b.hdist.get(), sizeof(double) * C);
}

static int host_logic() {
    const size_t n = 7 * 40, nw = 7 * 41;
    {
        Blocks b;
        CHECK(b.ensure(3, n, nw) == AIY_OK && g_live == kBufs);
        CHECK(b.key.cap() == 3 * n && b.off.cap() == 3 * nw && b.wr.cap() == 3 * n &&
              b.part.cap() == 3 * 256 && b.flags.cap() == 3 && b.hdist.cap() == 3);
        touch(b, 3, n, nw);
        int* const key = b.key.get();
        CHECK(b.ensure(2, n, nw) == AIY_OK && b.key.get() == key && g_live == kBufs);  // reuse
        touch(b, 2, n, nw);
        CHECK(b.ensure(70, n, nw) == AIY_OK && g_live == kBufs && b.off.cap() == 70 * nw &&
              b.iters.cap() == 70);
        touch(b, 70, n, nw);
        CHECK(b.ensure(5, n, nw) == AIY_OK && b.off.cap() == 70 * nw);  // the largest C seen stays
        CHECK(b.ensure(0, n, nw) == AIY_OK && g_live == kBufs);
        // an allocation that fails part of the way: the status comes back, nothing leaks, and the
        // group is usable again afterwards
        for (int k = 0; k < kBufs; ++k) {
            g_allocs = 0;
            g_fail_at = k;
            g_err.clear();
            if (b.ensure(1000, n, nw) != AIY_NO_MEMORY || g_err.empty()) {
                printf("FAILED allocation %d failing\n", k);
                return 1;
            }
            g_fail_at = -1;
            if (b.ensure(1000, n, nw) != AIY_OK || g_live != kBufs) {
                printf("FAILED recovery after allocation %d failed\n", k);
                return 1;
            }
            touch(b, 1000, n, nw);
            if (b.ensure(2000 + k, n, nw) != AIY_OK) return 1;  // (so that the next round reallocates)
            b = Blocks{};                                       // released by assignment
            if (g_live != 0) {
                printf("FAILED release after round %d: %d live\n", k, g_live);
                return 1;
            }
        }
        printf("ok a failing allocation at each of the %d positions\n", kBufs);
        CHECK(b.ensure((size_t)-1 / nw + 1, n, nw) == AIY_NO_MEMORY && g_live == 0);  // C·nw past size_t
        CHECK(b.ensure(2, n, n - 1) == AIY_NO_MEMORY && g_live == 0);                 // nw < n
        CHECK(b.ensure(5, n, nw) == AIY_OK && g_live == kBufs);
        Blocks c(std::move(b));  // a move leaves the source empty
        CHECK(b.key.get() == nullptr && b.hdist.get() == nullptr && c.key.cap() == 5 * n &&
              g_live == kBufs);
        touch(c, 5, n, nw);
    }  // the destructor frees
    CHECK(g_live == 0);
    return 0;
}

// the fit rule: the scripts' shape for both policy kinds within one CU's LDS, the layout's
// pieces inside the byte count
static int fit_rule() {
    using namespace aiy;
    CHECK(dist_batch_fits(7, 400, false) && dist_batch_fits(7, 400, true));
    CHECK(dist_batch_lds_bytes(7, 400, true) <= 160 * 1024);
    CHECK(dist_batch_lds_bytes(7, 400, false) ==
          8 * 2 * 2800 + 4 * 2808 + kDistBatchScratch);  // (7·401 = 2,807 offsets, padded)
    CHECK(dist_batch_fits(1, 2, false) && dist_batch_fits(16, 70, true));
    CHECK(!dist_batch_fits(7, 4000, false) && !dist_batch_fits(7, 4000, true));
    CHECK(!dist_batch_fits(17, 900, false) && !dist_batch_fits(0, 400, false) &&
          !dist_batch_fits(7, 1, false));
    // the largest Na that fits at N = 7: one more does not
    int64_t na = 2;
    while (dist_batch_fits(7, na + 1, true)) ++na;
    CHECK(dist_batch_lds_bytes(7, na, true) <= kDistBatchMaxLds &&
          dist_batch_lds_bytes(7, na + 1, true) > kDistBatchMaxLds && na > 400);
    return 0;
}

int main() {
    if (host_logic() || fit_rule()) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("FAILED a device is visible: run with HIP_VISIBLE_DEVICES=-1\n");
        return 1;
    }
    aiy::DistBatchBlocks real;
    g_err.clear();
    CHECK(real.ensure(63, 2800, 2807) == AIY_NO_MEMORY && !g_err.empty());
    CHECK(real.key.get() == nullptr && real.hiters.get() == nullptr);
    printf("done\n");
    return 0;
}
