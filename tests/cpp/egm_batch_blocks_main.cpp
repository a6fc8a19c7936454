// Stand-alone host program around the batched EGM solve's blocks (EgmBatchBlocksT,
// csrc/devbuf.hpp), built with -fsanitize=address,undefined by tests/test_egm_batch_cpu.py and
// run with no device visible.  The group is driven through a malloc-backed memory that can be
// told to fail at the k-th allocation, so the sanitizer sees every leak, double free and write
// past a block sized for C candidates; the real group is checked where every allocation fails.
// Prints one "ok" line per property; exits nonzero at the first one that does not hold.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "devbuf.hpp"

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

using Blocks = aiy::EgmBatchBlocksT<HostMem, HostMem>;

// what aiy_egm_solve_batch_dev does with blocks sized for C: every element written
static void touch(Blocks& b, size_t C) {
    for (size_t c = 0; c < C; ++c) {
        b.hrw.get()[c] = 0.01 * (double)c;
        b.hrw.get()[C + c] = 1.0;
        b.hiters.get()[c] = (long long)c;
        b.hdist.get()[c] = 0.5;
        b.hstatus.get()[c] = 0;
    }
    memcpy(b.rw.get(), b.hrw.get(), sizeof(double) * 2 * C);
    memcpy(b.iters.get(), b.hiters.get(), sizeof(long long) * C);
    memcpy(b.dist.get(), b.hdist.get(), sizeof(double) * C);
    memcpy(b.status.get(), b.hstatus.get(), sizeof(int) * C);
}

static int host_logic() {
    {
        Blocks b;
        CHECK(b.ensure(3) == AIY_OK && g_live == 8);
        CHECK(b.rw.cap() == 6 && b.hrw.cap() == 6 && b.iters.cap() == 3 && b.hstatus.cap() == 3);
        touch(b, 3);
        double* const rw = b.rw.get();
        CHECK(b.ensure(2) == AIY_OK && b.rw.get() == rw && g_live == 8);  // a smaller C reuses
        touch(b, 2);
        CHECK(b.ensure(70) == AIY_OK && g_live == 8 && b.rw.cap() == 140 && b.dist.cap() == 70);
        touch(b, 70);
        CHECK(b.ensure(0) == AIY_OK && g_live == 8);
        // an allocation that fails part of the way: the status comes back, nothing leaks, and the
        // group is usable again afterwards
        for (int k = 0; k < 8; ++k) {
            g_allocs = 0;
            g_fail_at = k;
            g_err.clear();
            if (b.ensure(1000) != AIY_NO_MEMORY || g_err.empty()) {
                printf("FAILED allocation %d failing\n", k);
                return 1;
            }
            g_fail_at = -1;
            if (b.ensure(1000) != AIY_OK || g_live != 8) {
                printf("FAILED recovery after allocation %d failed\n", k);
                return 1;
            }
            touch(b, 1000);
            if (b.ensure(2000 + k) != AIY_OK) return 1;  // (so that the next round reallocates)
            b = Blocks{};                                 // released by assignment
            if (g_live != 0) {
                printf("FAILED release after round %d: %d live\n", k, g_live);
                return 1;
            }
        }
        printf("ok a failing allocation at each of the 8 positions\n");
        CHECK(b.ensure((size_t)-1 / 2 + 1) == AIY_NO_MEMORY && g_live == 0);  // 2·C past size_t
        CHECK(b.ensure(5) == AIY_OK && g_live == 8);
        Blocks c(std::move(b));  // a move leaves the source empty
        CHECK(b.rw.get() == nullptr && b.hstatus.get() == nullptr && c.rw.cap() == 10 && g_live == 8);
        touch(c, 5);
    }  // the destructor frees
    CHECK(g_live == 0);
    return 0;
}

int main() {
    if (host_logic()) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("FAILED a device is visible: run with HIP_VISIBLE_DEVICES=-1\n");
        return 1;
    }
    aiy::EgmBatchBlocks real;
    g_err.clear();
    CHECK(real.ensure(63) == AIY_NO_MEMORY && !g_err.empty());
    CHECK(real.rw.get() == nullptr && real.hiters.get() == nullptr);
    printf("done\n");
    return 0;
}
