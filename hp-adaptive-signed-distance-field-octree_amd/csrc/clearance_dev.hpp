// What the kernels of clearance.hip (one pose) and clearance_batch.hip (many) share: the workgroup's shape and B's walk stack in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hpsdf {

namespace {

constexpr unsigned kClrThreads = 256;

inline uint32_t clrBlocks(uint32_t n) { return (n + kClrThreads - 1) / kClrThreads; }

// boundsWalkRange's Stack in LDS: level d of this lane at [d * kClrThreads + lane]
struct LdsClrStack {
    uint32_t* f;
    uint8_t* m;
    __device__ __forceinline__ uint32_t first(int d) const { return f[d * kClrThreads]; }
    __device__ __forceinline__ uint32_t mask(int d) const { return m[d * kClrThreads]; }
    __device__ __forceinline__ void setFirst(int d, uint32_t v) { f[d * kClrThreads] = v; }
    __device__ __forceinline__ void setMask(int d, uint32_t v) { m[d * kClrThreads] = (uint8_t)v; }
};

}  // namespace

}  // namespace hpsdf
