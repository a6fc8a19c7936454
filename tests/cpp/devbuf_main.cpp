// Stand-alone host program around csrc/devbuf.hpp (tests/test_host_layer_cpu.py builds it with
// -fsanitize=address,undefined and runs it with no device visible).  The buffer logic is driven
// through a malloc-backed memory that can be told to fail, so the sanitizer sees every leak and
// double free; DevBuf / PinnedBuf themselves are checked where every allocation fails.
// Prints one "ok" line per property; exits nonzero at the first one that does not hold.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

static int host_logic() {
    using B = aiy::Buf<int, HostMem>;
    {
        B b;
        bool fresh = false;
        CHECK(b.ensure(10, &fresh) == AIY_OK && fresh && b.cap() == 10 && g_live == 1);
        int* const p = b.get();
        for (int q = 0; q < 10; ++q) p[q] = q;  // (the sanitizer checks the extent)
        CHECK(b.ensure(5, &fresh) == AIY_OK && !fresh && b.get() == p && b.cap() == 10);
        CHECK(b.ensure(10, &fresh) == AIY_OK && !fresh && b.get() == p);
        CHECK(b.ensure(20, &fresh) == AIY_OK && fresh && b.cap() == 20 && g_live == 1);
        b.get()[19] = 1;
        g_oom = true;
        g_err.clear();
        CHECK(b.ensure(40, &fresh) == AIY_NO_MEMORY && !fresh && !g_err.empty());
        CHECK(b.get() == nullptr && b.cap() == 0 && g_live == 0);  // left empty, old memory freed
        CHECK(b.ensure(40) == AIY_NO_MEMORY && b.get() == nullptr);
        g_oom = false;
        CHECK(b.ensure(40, &fresh) == AIY_OK && fresh && b.cap() == 40);  // reusable
        CHECK(b.ensure((size_t)-1 / 2) == AIY_NO_MEMORY && g_live == 0);  // bytes past size_t
        CHECK(b.ensure(0, &fresh) == AIY_OK && fresh && b.cap() == 1 && b.get() != nullptr);
        b.release();
        CHECK(b.get() == nullptr && b.cap() == 0 && g_live == 0);
        b.release();  // idempotent
        CHECK(b.get() == nullptr && g_live == 0);
        CHECK(b.ensure(3) == AIY_OK);
        int* const q = b.get();
        B c(std::move(b));  // a move leaves the source empty
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == q && c.cap() == 3 && g_live == 1);
        CHECK(b.ensure(7) == AIY_OK && g_live == 2);
        b = std::move(c);  // move assignment frees what the target held
        CHECK(c.get() == nullptr && c.cap() == 0 && b.get() == q && b.cap() == 3 && g_live == 1);
        b = B{};  // released by assignment
        CHECK(b.get() == nullptr && g_live == 0);
        CHECK(b.ensure(2) == AIY_OK);
    }  // the destructor frees
    CHECK(g_live == 0);
    return 0;
}

template <class B>
static int no_device() {
    B b;
    bool fresh = true;
    g_err.clear();
    CHECK(b.ensure(1000, &fresh) == AIY_NO_MEMORY && !fresh && !g_err.empty());
    CHECK(b.get() == nullptr && b.cap() == 0);
    CHECK(b.ensure(0) == AIY_NO_MEMORY);
    b.release();
    b.release();
    B c(std::move(b));
    CHECK(b.get() == nullptr && c.get() == nullptr && c.cap() == 0);
    return 0;
}

int main() {
    if (host_logic()) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        printf("FAILED a device is visible: run with HIP_VISIBLE_DEVICES=-1\n");
        return 1;
    }
    if (no_device<aiy::DevBuf<double>>()) return 1;
    if (no_device<aiy::PinnedBuf<unsigned long long>>()) return 1;
    aiy::Events ev;
    CHECK(ev.create(2, 0) == AIY_HIP_ERROR && ev.size() == 0);  // none is left behind
    aiy::Events ev2(std::move(ev));
    CHECK(ev.size() == 0 && ev2.size() == 0);
    printf("done\n");
    return 0;
}
