// What hpsdf_extract_surface (surface.hip) and hpsdf_extract_surface_sparse (surface_sparse.hip) share.  The sparse call promises the
// dense call's mesh bit for bit, so everything both must agree on is written here once: the packed case table and its decode, the
// vertex arithmetic (edge_vertex.hpp, included here), the wave helpers, the check of the lattice arguments (lattice_check.hpp, included here: QueryBounds' grid entries
// share it) and the host scaffolding of a call (events, the malloc'd outputs; device memory and rocPRIM's two-call pattern are
// dev_pool.hpp's, which Integrate shares).  Included by those two units and by the dual call's (surface_dual.hip: same
// lattice, same scaffolding) only; each gets its own __constant__ copies.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "dev_pool.hpp"
#include "edge_vertex.hpp"
#include "host_call.hpp"
#include "lattice_check.hpp"
#include "runtime.hpp"
#include "surface_table.hpp"
#include "hpsdf.h"

namespace hpsdf {

namespace {

// ---- case table ------------------------------------------------------------------------------------------------------------------

struct PackedCases {
    uint64_t v[256];
};
constexpr PackedCases packCases() {
    const SurfaceTable T = makeSurfaceTable();
    PackedCases p{};
    for (int i = 0; i < 256; ++i) p.v[i] = T.packed[i];
    return p;
}
constexpr bool tableFits() {  // 3 bits of count and 12 bits a triangle in 64
    const SurfaceTable T = makeSurfaceTable();
    for (int i = 0; i < 256; ++i)
        if (T.count[i] > kSurfaceMaxTris) return false;
    return T.faceFreeFans;
}
static_assert(tableFits(), "a case of the face-local rule needs more than kSurfaceMaxTris triangles, or a loop has no apex whose fan stays out of the faces");

__constant__ PackedCases kSurfaceCases = packCases();

// cube-local edge -> its lower corner and axis (surface_table.hpp's numbering)
__constant__ uint8_t kEdgeCorner[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
__constant__ uint8_t kEdgeAxis[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2};

constexpr unsigned kSurfThreads = 256;  // the workgroup of every kernel of both units

// the packed table into LDS (the caller synchronises)
__device__ __forceinline__ void stageCases(uint64_t* sCase) {
    for (unsigned c = threadIdx.x; c < 256u; c += kSurfThreads) sCase[c] = kSurfaceCases.v[c];
}

// A packed case (surface_table.hpp): bits 0-2 the triangle count, then the triangles' cube-local edges.  The edge of vertex m of
// triangle tr, as its lower corner (dx + 2 dy + 4 dz) and its axis:
__device__ __forceinline__ uint32_t caseEdge(uint64_t pk, uint32_t tr, int m) { return (uint32_t)(pk >> (3 + 12 * tr + 4 * m)) & 15u; }
__device__ __forceinline__ uint8_t caseCorner(uint64_t pk, uint32_t tr, int m) { return kEdgeCorner[caseEdge(pk, tr, m)]; }
__device__ __forceinline__ uint8_t caseAxis(uint64_t pk, uint32_t tr, int m) { return kEdgeAxis[caseEdge(pk, tr, m)]; }

// ---- vertex arithmetic (include/hpsdf.h): edgeVertex, edge_vertex.hpp (the dual call's host path shares it) -----------------------

// ---- wave helpers ------------------------------------------------------------------------------------------------------------------

// set bits of a ballot mask in the lanes below this one: the rank of this lane's bit among the wave's
__device__ __forceinline__ uint32_t rankBelow(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// sum of n over the wave's lanes below this one: the wave's inclusive sum less the lane's own
__device__ __forceinline__ uint32_t sumBelow(uint32_t n, uint32_t lane) {
    uint32_t incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += y;
    }
    return incl - n;
}

inline unsigned gridOf(uint64_t threads, unsigned cap = 65536) {
    const uint64_t b = (threads + kSurfThreads - 1) / kSurfThreads;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- host scaffolding of a call ----------------------------------------------------------------------------------------------------

// N events on the call's stream; a failure to create or record one only zeroes the times
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    bool ok = true;
    Events() {
        for (auto& x : e)
            if (hipEventCreate(&x) != hipSuccess) x = nullptr, ok = false;
        if (!ok) (void)hipGetLastError();
    }
    ~Events() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
    void mark(int i, hipStream_t s) {
        if (ok && hipEventRecord(e[i], s) != hipSuccess) ok = false;
    }
    double ms(int a, int b) const {
        float r = 0.0f;
        return ok && hipEventElapsedTime(&r, e[a], e[b]) == hipSuccess ? (double)r : 0.0;
    }
};

// the scan of both calls' counts (uint32 counts -> uint64 exclusive prefixes) in withTemp's form
constexpr const char* kPrefixScan = "rocprim::exclusive_scan";
inline auto prefixScan(const uint32_t* in, uint64_t* out, uint64_t count, hipStream_t s) {
    return [=](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, (uint64_t)0, (size_t)count, rocprim::plus<uint64_t>(), s);
    };
}

struct HostOut {  // a malloc'd output, released unless handed to the caller
    void* p = nullptr;
    ~HostOut() { std::free(p); }
};

// The mesh on its way to the caller: host arrays for V vertices and T triangles, their download, and the handing over
struct MeshOut {
    HostOut v, t;
    uint64_t V = 0, T = 0;
    int alloc(const char* what, uint64_t nVerts, uint64_t nTris) {
        V = nVerts, T = nTris;
        v.p = std::malloc(V * 3 * sizeof(double));
        t.p = std::malloc(T * 3 * sizeof(uint64_t));
        return v.p && t.p ? HPSDF_OK : fail(HPSDF_ERR_OUT_OF_MEMORY, std::string(what) + ": host allocation failed");
    }
    int download(const double* dVerts, const uint64_t* dTris, hipStream_t s) {
        HPSDF_HIP(hipMemcpyAsync(v.p, dVerts, V * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(t.p, dTris, T * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        return HPSDF_OK;
    }
    void handOver(double** verts, uint64_t* nVerts, uint64_t** tris, uint64_t* nTris) {
        *verts = (double*)v.p, *tris = (uint64_t*)t.p;
        v.p = nullptr, t.p = nullptr;
        *nVerts = V, *nTris = T;
    }
};

}  // namespace

}  // namespace hpsdf
