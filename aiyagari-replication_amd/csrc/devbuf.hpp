// Owners of what a workspace allocates: DevBuf<T> (device), PinnedBuf<T> (pinned host), Events.
// Non-copyable, movable (the source is left empty), freed by the destructor.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/aiyagari_hip.h"

namespace aiy {

int fail(int code, const char* fmt, ...);

// a Buf's memory: the two HIP allocators (a test substitutes malloc); not a policy to extend
struct DevMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, 0); }
    static void free(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;  // elements

public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        Buf t(std::move(o));  // (frees what this held when it goes)
        std::swap(p_, t.p_);
        std::swap(cap_, t.cap_);
        return *this;
    }
    ~Buf() { release(); }
    // Room for n elements: nothing when the capacity suffices, else the old memory is freed and
    // max(n, 1) elements allocated, contents undefined; *fresh (nullable) tells which, so the
    // caller can fill the new memory or drop what it cached about the old.  On failure
    // AIY_NO_MEMORY, and the buffer is empty.
    int ensure(size_t n, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        if (p_ && cap_ >= n) return AIY_OK;
        release();
        const size_t m = n ? n : 1;
        void* q = nullptr;
        const hipError_t e = m > SIZE_MAX / sizeof(T) ? hipErrorOutOfMemory
                                                      : Mem::alloc(&q, m * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();  // reported here, not by the next launch's check
            return fail(AIY_NO_MEMORY, "allocating %zu x %zu bytes failed: %s", m, sizeof(T),
                        hipGetErrorString(e));
        }
        p_ = static_cast<T*>(q);
        cap_ = m;
        if (fresh) *fresh = true;
        return AIY_OK;
    }
    void release() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
};
template <class T>
using DevBuf = Buf<T, DevMem>;
template <class T>
using PinnedBuf = Buf<T, PinnedMem>;

// batched EGM solve (aiy_egm_solve_batch_dev): the per-candidate inputs and results on the
// device and their pinned copies, sized for the largest C seen (DM / PM: the two memories)
template <class DM, class PM>
struct EgmBatchBlocksT {
    Buf<double, DM> rw;        // device [2][C]: r then w
    Buf<long long, DM> iters;  // device [C]
    Buf<double, DM> dist;      // device [C]
    Buf<int, DM> status;       // device [C]
    Buf<double, PM> hrw;       // pinned [2][C]
    Buf<long long, PM> hiters;
    Buf<double, PM> hdist;
    Buf<int, PM> hstatus;
    // room for C candidates; on failure the status of the first allocation that failed (what
    // was allocated before it stays owned and is reused or freed as usual)
    int ensure(size_t C) {
        if (C > SIZE_MAX / 2) return fail(AIY_NO_MEMORY, "%zu candidates", C);
        int rc = rw.ensure(2 * C);
        if (rc == AIY_OK) rc = iters.ensure(C);
        if (rc == AIY_OK) rc = dist.ensure(C);
        if (rc == AIY_OK) rc = status.ensure(C);
        if (rc == AIY_OK) rc = hrw.ensure(2 * C);
        if (rc == AIY_OK) rc = hiters.ensure(C);
        if (rc == AIY_OK) rc = hdist.ensure(C);
        if (rc == AIY_OK) rc = hstatus.ensure(C);
        return rc;
    }
};
using EgmBatchBlocks = EgmBatchBlocksT<DevMem, PinnedMem>;

// batched histogram solve (aiy_dist_stationary_batch_dev): the candidates' plans (keys, run
// offsets, lottery weights), flags, results and partial sums of K on the device and the pinned
// copies of what the host reads, sized for the largest C seen at the workspace's (N, Na)
template <class DM, class PM>
struct DistBatchBlocksT {
    Buf<int, DM> key;          // device [C][N][Na]
    Buf<int, DM> off;          // device [C][N][Na+1]
    Buf<double, DM> wr;        // device [C][N][Na]
    Buf<double, DM> part;      // device [C][256]
    Buf<unsigned, DM> flags;   // device [C]
    Buf<long long, DM> iters;  // device [C]
    Buf<double, DM> dist;      // device [C]
    Buf<unsigned, PM> hflags;  // pinned [C]
    Buf<long long, PM> hiters;
    Buf<double, PM> hdist;
    // room for C candidates of n = N·Na states and nw = N·(Na+1) offsets; on failure the status
    // of the first allocation that failed (what was allocated before it stays owned and is
    // reused or freed as usual)
    int ensure(size_t C, size_t n, size_t nw) {
        if (nw < n || (nw && C > SIZE_MAX / nw) || C > SIZE_MAX / 256)
            return fail(AIY_NO_MEMORY, "%zu candidates of %zu states", C, n);
        int rc = key.ensure(C * n);
        if (rc == AIY_OK) rc = off.ensure(C * nw);
        if (rc == AIY_OK) rc = wr.ensure(C * n);
        if (rc == AIY_OK) rc = part.ensure(C * 256);
        if (rc == AIY_OK) rc = flags.ensure(C);
        if (rc == AIY_OK) rc = iters.ensure(C);
        if (rc == AIY_OK) rc = dist.ensure(C);
        if (rc == AIY_OK) rc = hflags.ensure(C);
        if (rc == AIY_OK) rc = hiters.ensure(C);
        if (rc == AIY_OK) rc = hdist.ensure(C);
        return rc;
    }
};
using DistBatchBlocks = DistBatchBlocksT<DevMem, PinnedMem>;

// events created together and destroyed with their owner
class Events {
    std::vector<hipEvent_t> ev_;

public:
    Events() = default;
    Events(Events&& o) noexcept : ev_(std::exchange(o.ev_, {})) {}
    Events& operator=(Events&& o) noexcept {
        Events t(std::move(o));
        ev_.swap(t.ev_);
        return *this;
    }
    ~Events() { release(); }
    int create(int n, unsigned flags) {  // AIY_HIP_ERROR on failure, leaving none
        release();
        ev_.resize(n, nullptr);
        for (hipEvent_t& e : ev_)
            if (hipEventCreateWithFlags(&e, flags) != hipSuccess) {
                release();
                return fail(AIY_HIP_ERROR, "hipEventCreate failed");
            }
        return AIY_OK;
    }
    void release() {
        for (hipEvent_t e : ev_)
            if (e) (void)hipEventDestroy(e);
        ev_.clear();
    }
    hipEvent_t operator[](size_t q) const { return ev_[q]; }
    size_t size() const { return ev_.size(); }
};

}  // namespace aiy
