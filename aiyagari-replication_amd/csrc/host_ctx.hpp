// Library-owned device buffers of the host tier, cached per (device, shape), and the typed
// staging every host entry goes through.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aiyagari_hip.h"
#include "devbuf.hpp"

namespace aiy {

// name -> owned bytes in the memory Mem (devbuf.hpp; a test substitutes malloc).  Per name it is
// Buf::ensure's rule: reused while the capacity suffices, else freed and allocated as asked,
// contents undefined.
template <class Mem>
struct NamedBufs {
    std::map<std::string, Buf<unsigned char, Mem>> m;
    int get(const char* name, size_t bytes, void** out) {
        auto& b = m[name];
        const int rc = b.ensure(bytes);
        *out = b.get();
        return rc;
    }
    size_t bytes() const {
        size_t n = 0;
        for (const auto& kv : m) n += kv.second.cap();
        return n;
    }
};

// AIY_OK, or AIY_HIP_ERROR naming the copy
inline int copy_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return AIY_OK;
    return fail(AIY_HIP_ERROR, "hipMemcpyAsync (%s) failed: %s", what, hipGetErrorString(e));
}

// MATLAB N x Na column-major <-> [N][Na] row-major
template <class T>
void cm_to_rows(const T* cm, int64_t N, int64_t Na, T* rows) {
    for (int64_t j = 0; j < Na; ++j)
        for (int64_t i = 0; i < N; ++i) rows[i * Na + j] = cm[i + j * N];
}
template <class T>
void rows_to_cm(const T* rows, int64_t N, int64_t Na, T* cm) {
    for (int64_t j = 0; j < Na; ++j)
        for (int64_t i = 0; i < N; ++i) cm[i + j * N] = rows[i * Na + j];
}

// the staging's device: DevMem's allocator, the stream's copies and its wait (a test substitutes
// malloc, memcpy and nothing)
struct DevStream : DevMem {
    static hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                           hipStream_t st) {
        return hipMemcpyAsync(dst, src, bytes, kind, st);
    }
    static hipError_t sync(hipStream_t st) { return hipStreamSynchronize(st); }
};

// Typed staging, sizes in elements.  Everything is enqueued on `st`; only sync and the two
// read-backs that convert a layout (they say so) wait.
// Host memory of an enqueued copy: the caller's arrays outlive the call, and what a helper
// converts on the way up gets storage of its own in `held`, one vector per copy, released by
// the next sync.  No host staging is reused between two enqueued copies.
template <class Dev>
struct Staging {
    hipStream_t st = nullptr;
    NamedBufs<Dev> bufs;
    std::vector<std::shared_ptr<void>> held;  // host sources of the uploads in flight

    // room: the buffer `name` with room for n elements.
    template <class T>
    int room(const char* name, size_t n, T** dev) {
        return bufs.get(name, n * sizeof(T), (void**)dev);
    }
    // up: room, then host -> device.
    template <class T>
    int up(const char* name, const T* host, size_t n, T** dev) {
        const int rc = room(name, n, dev);
        if (rc != AIY_OK) return rc;
        return copy_status(Dev::copy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice, st), name);
    }
    // down: device -> host.
    template <class T>
    int down(T* host, const T* dev, size_t n) {
        return copy_status(Dev::copy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st),
                           "read-back");
    }
    // sync: waits for the stream, then lets go of the uploads' host sources.
    int sync() {
        const hipError_t e = Dev::sync(st);
        held.clear();
        if (e == hipSuccess) return AIY_OK;
        return fail(AIY_HIP_ERROR, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    // up_own: up from a vector the staging keeps until the next sync.
    template <class T>
    int up_own(const char* name, std::vector<T> v, T** dev) {
        auto own = std::make_shared<std::vector<T>>(std::move(v));
        held.push_back(own);
        return up(name, own->data(), own->size(), dev);
    }
    // bcast: room for C blocks of n elements, block 0 from the host, blocks 1..C-1 from block 0.
    template <class T>
    int bcast(const char* name, const T* host, size_t n, int64_t C, T** dev) {
        const int rc = room(name, n * (size_t)C, dev);
        if (rc != AIY_OK) return rc;
        hipError_t e = Dev::copy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice, st);
        for (int64_t q = 1; q < C && e == hipSuccess; ++q)
            e = Dev::copy(*dev + q * n, *dev, n * sizeof(T), hipMemcpyDeviceToDevice, st);
        return copy_status(e, name);
    }
    // up_rows: C arrays N x Na column-major, up as [C][N][Na] rows.
    template <class T>
    int up_rows(const char* name, const T* cm, int64_t N, int64_t Na, int64_t C, T** dev) {
        const size_t n = (size_t)N * Na;
        std::vector<T> rows(n * (size_t)C);
        for (int64_t q = 0; q < C; ++q) cm_to_rows(cm + q * n, N, Na, rows.data() + q * n);
        return up_own(name, std::move(rows), dev);
    }
    // down_rows: [C][N][Na] rows back as C arrays N x Na column-major (synchronises).
    template <class T>
    int down_rows(T* cm, const T* dev, int64_t N, int64_t Na, int64_t C) {
        const size_t n = (size_t)N * Na;
        std::vector<T> rows(n * (size_t)C);
        int rc = down(rows.data(), dev, rows.size());
        if (rc == AIY_OK) rc = sync();
        if (rc != AIY_OK) return rc;
        for (int64_t q = 0; q < C; ++q) rows_to_cm(rows.data() + q * n, N, Na, cm + q * n);
        return AIY_OK;
    }
};

// The host tier's staging cap (bytes of device memory one chunk of a chunked host entry may
// ask for): aiy_dense_solve_batch and aiy_ssj_jacobian_batch process their C systems or economies
// in chunks of at most max(1, kBatchStageBytes / (bytes per system or economy)) when the caller
// passes chunk = 0.
constexpr size_t kBatchStageBytes = (size_t)4 << 30;

struct HostCtx : Staging<DevStream> {
    aiy_ws* ws = nullptr;
    ~HostCtx();
};

int get_ctx(int64_t N, int64_t Na, int64_t Nl, HostCtx** out);
std::mutex& host_mutex();
int check_grid(const double* a, int64_t Na);
int check_grid_strict(const double* a, int64_t Na);
int stage_common(HostCtx* c, const double* a, const double* s, const double* P, int64_t N,
                 int64_t Na, double** da, double** ds, double** dP);
// C policies' MATLAB indices (1-based; N x Na column-major, or Na x N when !vfi_layout) as the
// kernels' [C][N][Na] 0-based rows; NULL: zeros
std::vector<int> idx_rows0(const int32_t* idx1, int vfi_layout, int64_t N, int64_t Na,
                           int64_t C = 1);
// MATLAB's 4 x 4 transition matrix (column-major) as rows: out[4*i + m] = P(i, m)
void p_rows(const double* P, double out[16]);
// zi_shock as the kernels' int8, n values each 0 (good) or 1 (bad); anything else is AIY_BAD_ARG
int zi_to_i8(const double* zi_shock, size_t n, std::vector<int8_t>& out);

}  // namespace aiy
