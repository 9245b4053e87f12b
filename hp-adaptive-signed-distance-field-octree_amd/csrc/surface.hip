// hpsdf_extract_surface: marching cubes over a uniform lattice of a tree's values (no reference counterpart; include/hpsdf.h states
// the lattice, the ordering and the arithmetic).
//
//   1. lattice_query_kernel (kernels.hip): every lattice value, 8 bytes a point, through Query's own queryPoint;
//   2. surf_edge_words_kernel: one wave per 64 edge ids (edge 3 L + axis belongs to its lower point L) -- a ballot of the
//      crossing edges is the word, its popcount the word's vertex count;  surf_tri_count_kernel: one wave per 64 cubes (cube order
//      Q = i + n0 (j + n1 k)), the tile's triangle count from the case table;
//   3. rocprim exclusive scans of both counts (64-bit);
//   4. surf_vertex_kernel: a crossing edge's vertex id is its word's prefix + its rank in the word (mbcnt);  surf_tri_kernel: a cube's
//      first triangle is its tile's prefix + the wave's exclusive sum before it, and the vertex id of each of its edges is found the same
//      way from the bit words (an edge of the cube can belong to a word far from the cube's own tile).
// No atomics: every output position is a prefix, so the output is deterministic.  Scratch (one allocation, freed before returning):
// values 8 B a point, words + counts + prefixes 3 x 20 B per 64 points, tiles 12 B per 64 cubes, the scans' temporary storage.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include <rocprim/device/device_scan.hpp>

#include "device_types.hpp"
#include "launch.hpp"
#include "runtime.hpp"
#include "surface_table.hpp"
#include "hpsdf.h"

namespace hpsdf {

namespace {

struct PackedCases {
    uint64_t v[256];
};
constexpr PackedCases packCases() {
    const SurfaceTable T = makeSurfaceTable();
    PackedCases p{};
    for (int i = 0; i < 256; ++i) p.v[i] = T.packed[i];
    return p;
}
constexpr bool tableFits() {
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

constexpr unsigned kSurfBlock = 256;
constexpr unsigned kSurfMaxGrid = 8192;

unsigned surfGrid(uint64_t threads) {
    const uint64_t b = (threads + kSurfBlock - 1) / kSurfBlock;
    return (unsigned)(b < 1 ? 1 : (b > kSurfMaxGrid ? kSurfMaxGrid : b));
}

struct SurfArgs {
    SurfaceLattice g;
    double iso;
    uint64_t nEdges;  // 3 nPts
    uint64_t nWords;  // ceil(nEdges / 64)
    uint64_t nCubes;
    uint64_t nTiles;  // ceil(nCubes / 64)
};

// the exact ballot mask of lanes below this one: the rank of a set bit among the wave's
__device__ __forceinline__ uint32_t rankBelow(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ bool edgeCrosses(const double* __restrict__ v, const SurfArgs& A, uint64_t e) {
    if (e >= A.nEdges) return false;
    const uint32_t L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
    const uint32_t i = L % A.g.np[0], r = L / A.g.np[0], j = r % A.g.np[1], k = r / A.g.np[1];
    const uint32_t idx = a == 0 ? i : (a == 1 ? j : k);
    if (idx >= A.g.n[a]) return false;  // the edge would leave the lattice
    const uint32_t stride = a == 0 ? 1u : (a == 1 ? A.g.np[0] : A.g.np[0] * A.g.np[1]);
    return (v[L] < A.iso) != (v[L + stride] < A.iso);
}

__global__ __launch_bounds__(kSurfBlock) void surf_edge_words_kernel(const double* __restrict__ v, SurfArgs A, uint64_t* __restrict__ words,
                                                                     uint32_t* __restrict__ counts) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfBlock + threadIdx.x; e < total; e += stride) {  // wave-uniform: total is whole waves
        const uint64_t mask = __ballot(edgeCrosses(v, A, e));
        if ((threadIdx.x & 63u) == 0) {
            words[e >> 6] = mask;
            counts[e >> 6] = (uint32_t)__popcll(mask);
        }
    }
}

// case index of cube (i, j, k) whose lower corner is lattice point L0
__device__ __forceinline__ uint32_t cubeCase(const double* __restrict__ v, const SurfArgs& A, uint32_t L0) {
    const uint32_t sy = A.g.np[0], sz = A.g.np[0] * A.g.np[1];
    const uint32_t off[8] = {0u, 1u, sy, sy + 1u, sz, sz + 1u, sz + sy, sz + sy + 1u};
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) c |= (v[L0 + off[b]] < A.iso ? 1u : 0u) << b;
    return c;
}

__device__ __forceinline__ uint32_t cubeBase(const SurfArgs& A, uint64_t q) {
    const uint32_t Q = (uint32_t)q;
    const uint32_t i = Q % A.g.n[0], r = Q / A.g.n[0], j = r % A.g.n[1], k = r / A.g.n[1];
    return i + A.g.np[0] * (j + A.g.np[1] * k);
}

__device__ __forceinline__ void stageCases(uint64_t* sCase) {
    for (unsigned c = threadIdx.x; c < 256u; c += kSurfBlock) sCase[c] = kSurfaceCases.v[c];
    __syncthreads();
}

__global__ __launch_bounds__(kSurfBlock) void surf_tri_count_kernel(const double* __restrict__ v, SurfArgs A, uint32_t* __restrict__ counts) {
    __shared__ uint64_t sCase[256];
    stageCases(sCase);
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfBlock;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfBlock + threadIdx.x; q < total; q += stride) {
        uint32_t n = 0;
        if (q < A.nCubes) n = (uint32_t)(sCase[cubeCase(v, A, cubeBase(A, q))] & 7u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if ((threadIdx.x & 63u) == 0) counts[q >> 6] = n;
    }
}

__global__ __launch_bounds__(kSurfBlock) void surf_vertex_kernel(const double* __restrict__ v, SurfArgs A, const uint64_t* __restrict__ words,
                                                                 const uint64_t* __restrict__ prefix, double* __restrict__ verts) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfBlock + threadIdx.x; e < total; e += stride) {
        const uint64_t word = words[e >> 6];  // (one address for the whole wave)
        if (word == 0) continue;              // wave-uniform
        const uint32_t lane = (uint32_t)(e & 63u);
        if (!((word >> lane) & 1u)) continue;
        const uint64_t id = prefix[e >> 6] + (uint64_t)rankBelow(word & ((1ull << lane) - 1ull));
        const uint32_t L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
        const uint32_t idx[3] = {L % A.g.np[0], (L / A.g.np[0]) % A.g.np[1], (L / A.g.np[0]) / A.g.np[1]};
        const uint32_t s = a == 0 ? 1u : (a == 1 ? A.g.np[0] : A.g.np[0] * A.g.np[1]);
        const double va = v[L], vb = v[L + s];
        const double t = (A.iso - va) / (vb - va);
        double p[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = A.g.lo[d] + (double)idx[d] * A.g.h[d];
        const double xb = A.g.lo[a] + (double)(idx[a] + 1u) * A.g.h[a];
        p[a] = p[a] + t * (xb - p[a]);
        verts[3 * id] = p[0];
        verts[3 * id + 1] = p[1];
        verts[3 * id + 2] = p[2];
    }
}

__global__ __launch_bounds__(kSurfBlock) void surf_tri_kernel(const double* __restrict__ v, SurfArgs A, const uint64_t* __restrict__ words,
                                                              const uint64_t* __restrict__ vprefix, const uint64_t* __restrict__ tprefix,
                                                              uint64_t* __restrict__ tris) {
    __shared__ uint64_t sCase[256];
    stageCases(sCase);
    const uint32_t sy = A.g.np[0], sz = A.g.np[0] * A.g.np[1];
    const uint32_t cornerOff[8] = {0u, 1u, sy, sy + 1u, sz, sz + 1u, sz + sy, sz + sy + 1u};
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfBlock;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfBlock + threadIdx.x; q < total; q += stride) {
        uint64_t pk = 0;
        uint32_t L0 = 0;
        if (q < A.nCubes) {
            L0 = cubeBase(A, q);
            pk = sCase[cubeCase(v, A, L0)];
        }
        const uint32_t n = (uint32_t)(pk & 7u);
        uint32_t incl = n;  // inclusive sum over the wave's lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += y;
        }
        if (n == 0) continue;
        const uint64_t first = tprefix[q >> 6] + (uint64_t)(incl - n);
        for (uint32_t tr = 0; tr < n; ++tr) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const uint32_t le = (uint32_t)(pk >> (3 + 12 * tr + 4 * m)) & 15u;
                const uint64_t ge = 3u * (uint64_t)(L0 + cornerOff[kEdgeCorner[le]]) + kEdgeAxis[le];
                const uint64_t w = words[ge >> 6];
                const uint32_t bit = (uint32_t)(ge & 63u);
                tris[3 * (first + tr) + m] = vprefix[ge >> 6] + (uint64_t)__popcll(w & ((1ull << bit) - 1ull));
            }
        }
    }
}

size_t alignUp(size_t x) { return (x + 255) & ~(size_t)255; }

// the f32 containment test of queryPoint (leaf_eval.hpp, Octree.cpp:665-668) on one coordinate
bool inRoot(const TreeDev& t, int a, double x) {
    const float f = (float)((x - t.rootCentre[a]) * t.rootInvSizes[a]);
    return f >= -0.5f && f <= 0.5f;
}

int oom(const char* what) { return fail(HPSDF_ERR_OUT_OF_MEMORY, std::string("hpsdf_extract_surface: out of device memory (") + what + ")"); }

struct HostOut {  // malloc'd outputs, released unless handed to the caller
    void* p = nullptr;
    ~HostOut() { std::free(p); }
};

// per-phase device times of this thread's last call (hpsdf_surface_last_timings), from events on the context stream
thread_local double tLastMs[6] = {0, 0, 0, 0, 0, 0};

struct Events {
    hipEvent_t e[7] = {};
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
    float ms(int a, int b) const {
        float r = 0.0f;
        return ok && hipEventElapsedTime(&r, e[a], e[b]) == hipSuccess ? r : 0.0f;
    }
};

struct DevScratch {
    void* p = nullptr;
    ~DevScratch() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

}  // namespace hpsdf

using namespace hpsdf;

extern "C" {

int hpsdf_surface_case_table(int8_t* out) {
    if (!out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    static constexpr SurfaceTable T = makeSurfaceTable();
    std::memcpy(out, T.rows, sizeof T.rows);
    return HPSDF_OK;
}

int hpsdf_surface_last_timings(double* ms) {
    if (!ms) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    std::memcpy(ms, tLastMs, sizeof tLastMs);
    return HPSDF_OK;
}

int hpsdf_extract_surface(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3], double iso,
                          double** verts, uint64_t* nVerts, uint64_t** tris, uint64_t* nTris, double* values) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || !lo || !hi || !n || !verts || !nVerts || !tris || !nTris) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *verts = nullptr, *tris = nullptr, *nVerts = 0, *nTris = 0;
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    if (!std::isfinite(iso)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_extract_surface: iso must be finite");
    static const char* kAxis[3] = {"x", "y", "z"};
    SurfaceLattice g{};
    uint64_t nPts = 1, nCubes = 1;
    for (int a = 0; a < 3; ++a) {
        const std::string ax = std::string("hpsdf_extract_surface: axis ") + kAxis[a] + ": ";
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return fail(HPSDF_ERR_INVALID_ARGUMENT, ax + "lo and hi must be finite");
        if (!(lo[a] < hi[a])) return fail(HPSDF_ERR_INVALID_ARGUMENT, ax + "lo must be below hi");
        if (n[a] < 1) return fail(HPSDF_ERR_INVALID_ARGUMENT, ax + "n must be at least 1");
        nPts *= (uint64_t)n[a] + 1u;
        if (nPts > (1ull << 30)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_extract_surface: more than 2^30 lattice points");
        nCubes *= n[a];
        g.lo[a] = lo[a];
        g.h[a] = (hi[a] - lo[a]) / (double)n[a];
        g.n[a] = n[a];
        g.np[a] = n[a] + 1u;
        // the containment test is monotone along an axis: the two extreme lattice points decide for all of them
        const double last = g.lo[a] + (double)n[a] * g.h[a];
        if (!inRoot(t->dev, a, g.lo[a]) || !inRoot(t->dev, a, last))
            return fail(HPSDF_ERR_INVALID_ARGUMENT, ax + "the box leaves the tree's root (Query would return DBL_MAX there)");
    }
    g.nPts = (uint32_t)nPts;
    SurfArgs A{};
    A.g = g;
    A.iso = iso;
    A.nEdges = 3 * nPts;
    A.nWords = (A.nEdges + 63) / 64;
    A.nCubes = nCubes;
    A.nTiles = (nCubes + 63) / 64;

    HPSDF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // scratch: values | words | word counts | word prefixes | tile counts | tile prefixes | scan storage
    size_t tmpW = 0, tmpT = 0;
    HPSDF_HIP(rocprim::exclusive_scan(nullptr, tmpW, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(A.nWords + 1),
                                      rocprim::plus<uint64_t>(), s));
    HPSDF_HIP(rocprim::exclusive_scan(nullptr, tmpT, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)(A.nTiles + 1),
                                      rocprim::plus<uint64_t>(), s));
    const size_t oVals = 0, oWords = alignUp(oVals + nPts * 8), oWc = alignUp(oWords + A.nWords * 8),
                 oWp = alignUp(oWc + (A.nWords + 1) * 4), oTc = alignUp(oWp + (A.nWords + 1) * 8), oTp = alignUp(oTc + (A.nTiles + 1) * 4),
                 oTmp = alignUp(oTp + (A.nTiles + 1) * 8), total = oTmp + std::max(tmpW, tmpT) + 256;
    DevScratch scratch;
    {
        const hipError_t e = hipMalloc(&scratch.p, total);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            scratch.p = nullptr;
            return oom("scratch");
        }
        HPSDF_HIP(e);
    }
    char* base = (char*)scratch.p;
    double* dV = (double*)(base + oVals);
    uint64_t* dWords = (uint64_t*)(base + oWords);
    uint32_t* dWc = (uint32_t*)(base + oWc);
    uint64_t* dWp = (uint64_t*)(base + oWp);
    uint32_t* dTc = (uint32_t*)(base + oTc);
    uint64_t* dTp = (uint64_t*)(base + oTp);
    void* dTmp = base + oTmp;

    for (double& x : tLastMs) x = 0.0;
    Events ev;
    TreeDev td = t->dev;
    td.leftAssoc = reductionLeftAssoc(ctx);
    ev.mark(0, s);
    HPSDF_HIP(launchQueryLattice(s, td, ctx->dTables, g, dV));
    ev.mark(1, s);
    HPSDF_HIP(hipMemsetAsync(dWc + A.nWords, 0, 4, s));
    HPSDF_HIP(hipMemsetAsync(dTc + A.nTiles, 0, 4, s));
    hipLaunchKernelGGL(surf_edge_words_kernel, dim3(surfGrid(A.nWords * 64)), dim3(kSurfBlock), 0, s, dV, A, dWords, dWc);
    HPSDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(surf_tri_count_kernel, dim3(surfGrid(A.nTiles * 64)), dim3(kSurfBlock), 0, s, dV, A, dTc);
    HPSDF_HIP(hipGetLastError());
    ev.mark(2, s);
    HPSDF_HIP(rocprim::exclusive_scan(dTmp, tmpW, dWc, dWp, (uint64_t)0, (size_t)(A.nWords + 1), rocprim::plus<uint64_t>(), s));
    HPSDF_HIP(rocprim::exclusive_scan(dTmp, tmpT, dTc, dTp, (uint64_t)0, (size_t)(A.nTiles + 1), rocprim::plus<uint64_t>(), s));
    ev.mark(3, s);
    uint64_t counts[2] = {0, 0};
    HPSDF_HIP(hipMemcpyAsync(&counts[0], dWp + A.nWords, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipMemcpyAsync(&counts[1], dTp + A.nTiles, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipStreamSynchronize(s));
    const uint64_t V = counts[0], T = counts[1];

    HostOut hv, ht;
    DevScratch outs;
    if (T > 0) {
        hv.p = std::malloc(V * 3 * sizeof(double));
        ht.p = std::malloc(T * 3 * sizeof(uint64_t));
        if (!hv.p || !ht.p) return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_extract_surface: host allocation failed");
        const size_t oT = alignUp(V * 3 * sizeof(double));
        const hipError_t e = hipMalloc(&outs.p, oT + T * 3 * sizeof(uint64_t));
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            outs.p = nullptr;
            return oom("outputs");
        }
        HPSDF_HIP(e);
        double* dVerts = (double*)outs.p;
        uint64_t* dTris = (uint64_t*)((char*)outs.p + oT);
        ev.mark(4, s);
        hipLaunchKernelGGL(surf_vertex_kernel, dim3(surfGrid(A.nWords * 64)), dim3(kSurfBlock), 0, s, dV, A, dWords, dWp, dVerts);
        HPSDF_HIP(hipGetLastError());
        hipLaunchKernelGGL(surf_tri_kernel, dim3(surfGrid(A.nTiles * 64)), dim3(kSurfBlock), 0, s, dV, A, dWords, dWp, dTp, dTris);
        HPSDF_HIP(hipGetLastError());
        ev.mark(5, s);
        HPSDF_HIP(hipMemcpyAsync(hv.p, dVerts, V * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(ht.p, dTris, T * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    }
    if (values) HPSDF_HIP(hipMemcpyAsync(values, dV, nPts * sizeof(double), hipMemcpyDeviceToHost, s));
    ev.mark(6, s);
    HPSDF_HIP(hipStreamSynchronize(s));
    tLastMs[0] = ev.ms(0, 1), tLastMs[1] = ev.ms(1, 2), tLastMs[2] = ev.ms(2, 3);
    if (T > 0) tLastMs[3] = ev.ms(4, 5);
    tLastMs[4] = ev.ms(T > 0 ? 5 : 3, 6);
    tLastMs[5] = ev.ms(0, 6);
    if (T > 0) {
        *verts = (double*)hv.p, *tris = (uint64_t*)ht.p;
        hv.p = nullptr, ht.p = nullptr;
        *nVerts = V, *nTris = T;
    }
    return HPSDF_OK;
    HPSDF_CATCH
}

}  // extern "C"
