// Library-owned device buffers of the host tier, cached per (device, shape).  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <map>
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

int copy_status(hipError_t e, const char* what);  // AIY_OK, or AIY_HIP_ERROR naming the copy

struct HostCtx {
    aiy_ws* ws = nullptr;
    hipStream_t st = nullptr;
    NamedBufs<DevMem> bufs;
    int buf(const char* name, size_t bytes, void** out) { return bufs.get(name, bytes, out); }
    // Typed staging, sizes in elements; everything is enqueued on `st` and nothing waits.
    // room: the buffer `name` with room for n elements.
    template <class T>
    int room(const char* name, size_t n, T** dev) {
        return buf(name, n * sizeof(T), (void**)dev);
    }
    // up: room, then host -> device.
    template <class T>
    int up(const char* name, const T* host, size_t n, T** dev) {
        const int rc = room(name, n, dev);
        if (rc != AIY_OK) return rc;
        return copy_status(hipMemcpyAsync(*dev, host, n * sizeof(T), hipMemcpyHostToDevice, st),
                           name);
    }
    // down: device -> host.
    template <class T>
    int down(T* host, const T* dev, size_t n) {
        return copy_status(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st),
                           "read-back");
    }
    ~HostCtx();
};

int get_ctx(int64_t N, int64_t Na, int64_t Nl, HostCtx** out);
std::mutex& host_mutex();
void cm_to_rows(const double* cm, int64_t N, int64_t Na, double* rows);
void rows_to_cm(const double* rows, int64_t N, int64_t Na, double* cm);
int check_grid(const double* a, int64_t Na);
int check_grid_strict(const double* a, int64_t Na);
int stage_common(HostCtx* c, const double* a, const double* s, const double* P, int64_t N,
                 int64_t Na, double** da, double** ds, double** dP);
// MATLAB's 4 x 4 transition matrix (column-major) as rows: out[4*i + m] = P(i, m)
void p_rows(const double* P, double out[16]);
// zi_shock as the kernels' int8, n values each 0 (good) or 1 (bad); anything else is AIY_BAD_ARG
int zi_to_i8(const double* zi_shock, size_t n, std::vector<int8_t>& out);

}  // namespace aiy
