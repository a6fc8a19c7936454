// Stand-alone host program around the host tier's name -> buffer map (csrc/host_ctx.hpp,
// NamedBufs; tests/test_host_layer_cpu.py builds it with -fsanitize=address,undefined).  The map
// is driven through a malloc-backed memory, so the sanitizer sees every leak, double free and
// write past a buffer's extent.  No device is needed and none is touched.
// Prints one "ok" line per property; exits nonzero at the first one that does not hold.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

int main() {
    if (named_bufs()) return 1;
    printf("done\n");
    return 0;
}
