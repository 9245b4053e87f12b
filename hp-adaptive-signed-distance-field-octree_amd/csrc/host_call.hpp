// The *_host entry points of capi_field.cpp and capi_tree.cpp (host arrays in, host arrays out): the context's cached device and pinned scratch, the list an
// entry names its arrays in, and the call that moves them by one of three paths.
#pragma once
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "runtime.hpp"

namespace hpsdf {

constexpr size_t kPinnedPathBytes = 1u << 20;  // below this, user memory is staged through the pinned buffer
constexpr size_t kZeroCopyBytes = 4096;        // below this the kernel works on the pinned buffer itself: a scalar
                                               // Query(pt) then costs a launch and a wait, not two copies as well
inline size_t alignUp(size_t b) { return (b + 255) & ~(size_t)255; }

inline int ensureHostScratch(hpsdf_ctx* ctx, size_t devBytes, size_t pinBytes) {
    if (ctx->hostDevCap < devBytes) {
        if (ctx->hostDev) HPSDF_HIP(hipFree(ctx->hostDev));
        ctx->hostDev = nullptr;
        ctx->hostDevCap = 0;
        size_t cap = 1u << 16;
        while (cap < devBytes) cap *= 2;
        HPSDF_HIP(hipMalloc((void**)&ctx->hostDev, cap));
        ctx->hostDevCap = cap;
    }
    if (ctx->hostPinCap < pinBytes) {
        if (ctx->hostPin) HPSDF_HIP(hipHostFree(ctx->hostPin));
        ctx->hostPin = nullptr;
        ctx->hostPinCap = 0;
        size_t cap = 1u << 16;
        while (cap < pinBytes) cap *= 2;
        HPSDF_HIP(hipHostMalloc((void**)&ctx->hostPin, cap, hipHostMallocDefault));
        ctx->hostPinCap = cap;
        void* dp = nullptr;
        ctx->hostPinDev = hipHostGetDevicePointer(&dp, ctx->hostPin, 0) == hipSuccess ? (char*)dp : nullptr;
    }
    return HPSDF_OK;
}

// The arrays of one host call.  in(), out() and inout() (copied both ways: rows the kernel leaves untouched keep the caller's values) take
// a host pointer and its element count and hand back the array's device pointer, typed; it is valid inside hostCall's `run`.  An output
// whose host pointer is null takes no slot, no scratch bytes and no copy, and its device pointer is null.  No allocation: the slots are here.
struct HostArrays {
    struct Slot {
        const void* src;  // host source (nullptr: output only)
        void* dst;        // host destination (nullptr: input only)
        size_t bytes;
        size_t off;  // where the array starts in the call's scratch, and there on the device (both set by hostCall)
        char* dev;
    };
    template <typename T>
    struct Dev {
        const Slot* slot;
        operator T*() const { return slot ? reinterpret_cast<T*>(slot->dev) : nullptr; }
    };
    template <typename T>
    Dev<const T> in(const T* src, size_t count) { return {add(src, nullptr, count * sizeof(T))}; }
    template <typename T>
    Dev<T> out(T* dst, size_t count) { return {dst ? add(nullptr, dst, count * sizeof(T)) : nullptr}; }
    template <typename T>
    Dev<T> inout(T* both, size_t count) { return {add(both, both, count * sizeof(T))}; }
    const Slot* add(const void* src, void* dst, size_t bytes) {
        if (used == kSlots) throw std::length_error("a host call with more arrays than HostArrays holds");
        slots[used] = Slot{src, dst, bytes, 0, nullptr};
        return &slots[used++];
    }
    HostArrays() = default;
    HostArrays(const HostArrays&) = delete;  // (a Dev points at its slot)
    static constexpr int kSlots = 10;        // hpsdf_cast_rays_host: three inputs, seven outputs
    Slot slots[kSlots];
    int used = 0;
    Slot* begin() { return slots; }
    Slot* end() { return slots + used; }
};
// One host call: the arrays with a source are copied to the device, `run` launches on the context stream, those with a destination come back.
template <typename Run>
int hostCall(hpsdf_ctx* ctx, HostArrays& list, Run&& run) {
    std::lock_guard<std::mutex> guard(ctx->hostLock);
    HPSDF_HIP(hipSetDevice(ctx->device));
    size_t total = 0;
    for (HostArrays::Slot& s : list) s.off = total, total += alignUp(s.bytes);
    const bool staged = total <= kPinnedPathBytes;
    int rc = ensureHostScratch(ctx, total, staged ? total : 0);
    if (rc) return rc;
    static const bool zeroCopyOff = std::getenv("HPSDF_NO_ZEROCOPY") != nullptr;  // measurement knob
    const bool zeroCopy = total <= kZeroCopyBytes && ctx->hostPinDev != nullptr && !zeroCopyOff;
    for (HostArrays::Slot& s : list) {
        s.dev = (zeroCopy ? ctx->hostPinDev : ctx->hostDev) + s.off;
        if (!s.src) continue;
        if (staged) std::memcpy(ctx->hostPin + s.off, s.src, s.bytes);
        if (!zeroCopy) HPSDF_HIP(hipMemcpyAsync(s.dev, staged ? ctx->hostPin + s.off : s.src, s.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run();
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    for (const HostArrays::Slot& s : list)
        if (s.dst && !zeroCopy)
            HPSDF_HIP(hipMemcpyAsync(staged ? (void*)(ctx->hostPin + s.off) : s.dst, s.dev, s.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HPSDF_HIP(hipStreamSynchronize(ctx->stream));
    for (const HostArrays::Slot& s : list)
        if (s.dst && staged) std::memcpy(s.dst, ctx->hostPin + s.off, s.bytes);
    return HPSDF_OK;
}

// The host call of n points in and one value a point out: run(const double* dXyz, double* dOut) launches on the context stream.
template <typename Run>
int hostRoundTrip(hpsdf_ctx* ctx, const double* xyz, size_t n, double* out, Run&& run) {
    if (n == 0) return HPSDF_OK;
    HostArrays arr;
    const auto dXyz = arr.in(xyz, n * 3);
    const auto dOut = arr.out(out, n);
    return hostCall(ctx, arr, [&] { return run(dXyz, dOut); });
}

// Up to how many points / rays a *_host call is answered on the calling thread.  The defaults are where the two paths cost the same on an
// MI355X box (tools/host_api_latency.py, profiles/r04_host_call_thresholds.txt): a launch round trip is ~15 us (~55 us for the mesh
// traversal), a point on the host 0.045 us (Query), 0.07 us (gradient), <= 9 us (a ray: up to 200 Query steps), ~23 us (mesh distance).
// HPSDF_HOST_QUERY_POINTS / _GRADIENT_POINTS / _RAYS / _MESH_POINTS override them (read once).
inline size_t hostLimit(const char* env, size_t dflt) {
    const char* e = std::getenv(env);
    if (!e) return dflt;
    const long v = std::atol(e);
    return v < 0 ? 0 : (size_t)v;
}
inline size_t hostQueryLimit() { static const size_t v = hostLimit("HPSDF_HOST_QUERY_POINTS", kHostQueryPoints); return v; }
inline size_t hostGradientLimit() { static const size_t v = hostLimit("HPSDF_HOST_GRADIENT_POINTS", kHostGradientPoints); return v; }
inline size_t hostRayLimit() { static const size_t v = hostLimit("HPSDF_HOST_RAYS", kHostRays); return v; }
inline size_t hostMeshLimit() { static const size_t v = hostLimit("HPSDF_HOST_MESH_POINTS", kHostMeshPoints); return v; }
// HPSDF_SMALL_QUERIES_ON_DEVICE=1 (read once) sends calls of a few points through query_few_kernel as before round 4: a measurement knob
inline bool smallQueriesOnHost() {
    static const bool on = [] {
        const char* e = std::getenv("HPSDF_SMALL_QUERIES_ON_DEVICE");
        return !(e && e[0] == '1');
    }();
    return on;
}

}  // namespace hpsdf
