// The device memory of one call and rocPRIM's two-call pattern on it: what hpsdf_extract_surface, hpsdf_extract_surface_sparse
// (through surface_common.hpp) and hpsdf_integrate_device (integrate.hip) take their arrays from.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "runtime.hpp"
#include "hpsdf.h"

namespace hpsdf {

namespace {

// The device memory of one call of the entry point `what`: what is live, the most that was, and everything freed when the call ends.
// The dense call takes one allocation and carves it; the sparse call takes and releases its arrays by name to keep the peak low.
struct DevPool {
    const char* what;
    std::vector<std::pair<void*, size_t>> live;
    size_t cur = 0, peak = 0;
    explicit DevPool(const char* w) : what(w) {}
    DevPool(const DevPool&) = delete;
    // HPSDF_OK, or the failure's code with its message set: running out of device memory names the array
    template <typename T>
    int alloc(T*& p, size_t bytes, const char* name) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes < 256 ? 256 : bytes);
        p = e == hipSuccess ? (T*)q : nullptr;
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            return fail(HPSDF_ERR_OUT_OF_MEMORY, std::string(what) + ": out of device memory (" + name + ")");
        }
        if (e != hipSuccess) return hipFail(e, "hipMalloc");
        live.emplace_back(q, bytes);
        cur += bytes;
        peak = cur > peak ? cur : peak;
        return HPSDF_OK;
    }
    template <typename T>
    void release(T*& p) {  // (the stream must have passed the array's last use)
        for (auto& x : live)
            if (x.first == (void*)p && p != nullptr) {
                (void)hipFree(x.first);
                cur -= x.second;
                x = live.back();
                live.pop_back();
                break;
            }
        p = nullptr;
    }
    ~DevPool() {
        for (auto& x : live) (void)hipFree(x.first);
    }
};

#define SURF_ALLOC(pool, ptr, bytes, name)                                     \
    do {                                                                       \
        if (const int rc_ = (pool).alloc((ptr), (bytes), (name))) return rc_; \
    } while (0)

// the status of a rocPRIM step behind a lambda: a failure names the primitive (`prim`, e.g. "rocprim::reduce"), not the lambda
inline int primStatus(hipError_t e, const char* prim) { return e == hipSuccess ? HPSDF_OK : hipFail(e, prim); }

// rocPRIM's two-call pattern: call(nullptr, bytes) asks for the size of the temporary storage, which then comes from the pool under
// `name`, and call(tmp, bytes) runs.  tmp stays the caller's to release (or to run the same call on other arrays first).
template <typename Call>
int withTemp(DevPool& pool, const char* prim, const char* name, void*& tmp, size_t& bytes, Call&& call) {
    bytes = 0;
    if (const int rc = primStatus(call(nullptr, bytes), prim)) return rc;
    SURF_ALLOC(pool, tmp, bytes, name);
    if (const int rc = primStatus(call(tmp, bytes), prim)) return rc;
    return HPSDF_OK;
}

}  // namespace

}  // namespace hpsdf
