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
// Case table, vertex arithmetic, wave helpers, argument checks and the call's host scaffolding: surface_common.hpp, shared with the sparse call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "device_types.hpp"
#include "launch.hpp"
#include "surface_common.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kSurfMaxGrid = 8192;

struct SurfArgs {
    SurfaceLattice g;
    double iso;
    uint64_t nEdges;  // 3 nPts
    uint64_t nWords;  // ceil(nEdges / 64)
    uint64_t nCubes;
    uint64_t nTiles;  // ceil(nCubes / 64)
};

__device__ __forceinline__ bool edgeCrosses(const double* __restrict__ v, const SurfArgs& A, uint64_t e) {
    if (e >= A.nEdges) return false;
    const uint32_t L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
    const uint32_t i = L % A.g.np[0], r = L / A.g.np[0], j = r % A.g.np[1], k = r / A.g.np[1];
    const uint32_t idx = a == 0 ? i : (a == 1 ? j : k);
    if (idx >= A.g.n[a]) return false;  // the edge would leave the lattice
    const uint32_t stride = a == 0 ? 1u : (a == 1 ? A.g.np[0] : A.g.np[0] * A.g.np[1]);
    return (v[L] < A.iso) != (v[L + stride] < A.iso);
}

__global__ __launch_bounds__(kSurfThreads) void surf_edge_words_kernel(const double* __restrict__ v, SurfArgs A, uint64_t* __restrict__ words,
                                                                     uint32_t* __restrict__ counts) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; e < total; e += stride) {  // wave-uniform: total is whole waves
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

__global__ __launch_bounds__(kSurfThreads) void surf_tri_count_kernel(const double* __restrict__ v, SurfArgs A, uint32_t* __restrict__ counts) {
    __shared__ uint64_t sCase[256];
    stageCases(sCase);
    __syncthreads();
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; q < total; q += stride) {
        uint32_t n = 0;
        if (q < A.nCubes) n = (uint32_t)(sCase[cubeCase(v, A, cubeBase(A, q))] & 7u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if ((threadIdx.x & 63u) == 0) counts[q >> 6] = n;
    }
}

__global__ __launch_bounds__(kSurfThreads) void surf_vertex_kernel(const double* __restrict__ v, SurfArgs A, const uint64_t* __restrict__ words,
                                                                 const uint64_t* __restrict__ prefix, double* __restrict__ verts) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; e < total; e += stride) {
        const uint64_t word = words[e >> 6];  // (one address for the whole wave)
        if (word == 0) continue;              // wave-uniform
        const uint32_t lane = (uint32_t)(e & 63u);
        if (!((word >> lane) & 1u)) continue;
        const uint64_t id = prefix[e >> 6] + (uint64_t)rankBelow(word & ((1ull << lane) - 1ull));
        const uint32_t L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
        const uint32_t idx[3] = {L % A.g.np[0], (L / A.g.np[0]) % A.g.np[1], (L / A.g.np[0]) / A.g.np[1]};
        const uint32_t s = a == 0 ? 1u : (a == 1 ? A.g.np[0] : A.g.np[0] * A.g.np[1]);
        const double va = v[L], vb = v[L + s];
        double p[3];
        edgeVertex(A.g.lo, A.g.h, idx, a, va, vb, A.iso, p);
        verts[3 * id] = p[0];
        verts[3 * id + 1] = p[1];
        verts[3 * id + 2] = p[2];
    }
}

__global__ __launch_bounds__(kSurfThreads) void surf_tri_kernel(const double* __restrict__ v, SurfArgs A, const uint64_t* __restrict__ words,
                                                              const uint64_t* __restrict__ vprefix, const uint64_t* __restrict__ tprefix,
                                                              uint64_t* __restrict__ tris) {
    __shared__ uint64_t sCase[256];
    stageCases(sCase);
    __syncthreads();
    const uint32_t sy = A.g.np[0], sz = A.g.np[0] * A.g.np[1];
    const uint32_t cornerOff[8] = {0u, 1u, sy, sy + 1u, sz, sz + 1u, sz + sy, sz + sy + 1u};
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; q < total; q += stride) {
        uint64_t pk = 0;
        uint32_t L0 = 0;
        if (q < A.nCubes) {
            L0 = cubeBase(A, q);
            pk = sCase[cubeCase(v, A, L0)];
        }
        const uint32_t n = (uint32_t)(pk & 7u);
        const uint32_t before = sumBelow(n, lane);  // (every lane takes part)
        if (n == 0) continue;
        const uint64_t first = tprefix[q >> 6] + (uint64_t)before;
        for (uint32_t tr = 0; tr < n; ++tr) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const uint64_t ge = 3u * (uint64_t)(L0 + cornerOff[caseCorner(pk, tr, m)]) + caseAxis(pk, tr, m);
                const uint64_t w = words[ge >> 6];
                const uint32_t bit = (uint32_t)(ge & 63u);
                tris[3 * (first + tr) + m] = vprefix[ge >> 6] + (uint64_t)__popcll(w & ((1ull << bit) - 1ull));
            }
        }
    }
}

// per-phase device times of this thread's last call (hpsdf_surface_last_timings), from events on the context stream
thread_local double tLastMs[6] = {0, 0, 0, 0, 0, 0};

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
    static const char* kWhat = "hpsdf_extract_surface";
    CheckedLattice cl{};
    if (const int rc = checkLattice(kWhat, kDenseLimits, t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, iso, &cl)) return rc;
    const uint64_t nPts = cl.nPts;
    SurfArgs A{};
    SurfaceLattice& g = A.g;
    for (int a = 0; a < 3; ++a) g.lo[a] = cl.lo[a], g.h[a] = cl.h[a], g.n[a] = cl.n[a], g.np[a] = cl.n[a] + 1u;
    g.nPts = (uint32_t)nPts;
    A.iso = iso;
    A.nEdges = 3 * nPts;
    A.nWords = (A.nEdges + 63) / 64;
    A.nCubes = cl.nCubes;
    A.nTiles = (cl.nCubes + 63) / 64;

    HPSDF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // scratch, one allocation: values | words | word counts | word prefixes | tile counts | tile prefixes | scan storage
    size_t tmpW = 0, tmpT = 0;
    if (const int rc = primStatus(prefixScan(nullptr, nullptr, A.nWords + 1, s)(nullptr, tmpW), kPrefixScan)) return rc;
    if (const int rc = primStatus(prefixScan(nullptr, nullptr, A.nTiles + 1, s)(nullptr, tmpT), kPrefixScan)) return rc;
    const size_t oVals = 0, oWords = alignUp(oVals + nPts * 8), oWc = alignUp(oWords + A.nWords * 8),
                 oWp = alignUp(oWc + (A.nWords + 1) * 4), oTc = alignUp(oWp + (A.nWords + 1) * 8), oTp = alignUp(oTc + (A.nTiles + 1) * 4),
                 oTmp = alignUp(oTp + (A.nTiles + 1) * 8), total = oTmp + std::max(tmpW, tmpT) + 256;
    DevPool pool(kWhat);
    char* base = nullptr;
    SURF_ALLOC(pool, base, total, "scratch");
    double* dV = (double*)(base + oVals);
    uint64_t* dWords = (uint64_t*)(base + oWords);
    uint32_t* dWc = (uint32_t*)(base + oWc);
    uint64_t* dWp = (uint64_t*)(base + oWp);
    uint32_t* dTc = (uint32_t*)(base + oTc);
    uint64_t* dTp = (uint64_t*)(base + oTp);
    void* dTmp = base + oTmp;

    for (double& x : tLastMs) x = 0.0;
    Events<7> ev;
    TreeDev td = t->dev;
    td.leftAssoc = reductionLeftAssoc(ctx);
    ev.mark(0, s);
    HPSDF_HIP(launchQueryLattice(s, td, ctx->dTables, A.g, dV));
    ev.mark(1, s);
    HPSDF_HIP(hipMemsetAsync(dWc + A.nWords, 0, 4, s));
    HPSDF_HIP(hipMemsetAsync(dTc + A.nTiles, 0, 4, s));
    hipLaunchKernelGGL(surf_edge_words_kernel, dim3(gridOf(A.nWords * 64, kSurfMaxGrid)), dim3(kSurfThreads), 0, s, dV, A, dWords, dWc);
    HPSDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(surf_tri_count_kernel, dim3(gridOf(A.nTiles * 64, kSurfMaxGrid)), dim3(kSurfThreads), 0, s, dV, A, dTc);
    HPSDF_HIP(hipGetLastError());
    ev.mark(2, s);
    if (const int rc = primStatus(prefixScan(dWc, dWp, A.nWords + 1, s)(dTmp, tmpW), kPrefixScan)) return rc;
    if (const int rc = primStatus(prefixScan(dTc, dTp, A.nTiles + 1, s)(dTmp, tmpT), kPrefixScan)) return rc;
    ev.mark(3, s);
    uint64_t counts[2] = {0, 0};
    HPSDF_HIP(hipMemcpyAsync(&counts[0], dWp + A.nWords, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipMemcpyAsync(&counts[1], dTp + A.nTiles, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipStreamSynchronize(s));
    const uint64_t V = counts[0], T = counts[1];

    MeshOut mesh;
    if (T > 0) {
        if (const int rc = mesh.alloc(kWhat, V, T)) return rc;
        const size_t oT = alignUp(V * 3 * sizeof(double));
        char* outs = nullptr;
        SURF_ALLOC(pool, outs, oT + T * 3 * sizeof(uint64_t), "outputs");
        double* dVerts = (double*)outs;
        uint64_t* dTris = (uint64_t*)(outs + oT);
        ev.mark(4, s);
        hipLaunchKernelGGL(surf_vertex_kernel, dim3(gridOf(A.nWords * 64, kSurfMaxGrid)), dim3(kSurfThreads), 0, s, dV, A, dWords, dWp, dVerts);
        HPSDF_HIP(hipGetLastError());
        hipLaunchKernelGGL(surf_tri_kernel, dim3(gridOf(A.nTiles * 64, kSurfMaxGrid)), dim3(kSurfThreads), 0, s, dV, A, dWords, dWp, dTp, dTris);
        HPSDF_HIP(hipGetLastError());
        ev.mark(5, s);
        if (const int rc = mesh.download(dVerts, dTris, s)) return rc;
    }
    if (values) HPSDF_HIP(hipMemcpyAsync(values, dV, nPts * sizeof(double), hipMemcpyDeviceToHost, s));
    ev.mark(6, s);
    HPSDF_HIP(hipStreamSynchronize(s));
    tLastMs[0] = ev.ms(0, 1), tLastMs[1] = ev.ms(1, 2), tLastMs[2] = ev.ms(2, 3);
    if (T > 0) tLastMs[3] = ev.ms(4, 5);
    tLastMs[4] = ev.ms(T > 0 ? 5 : 3, 6);
    tLastMs[5] = ev.ms(0, 6);
    if (T > 0) mesh.handOver(verts, nVerts, tris, nTris);
    return HPSDF_OK;
    HPSDF_CATCH
}

}  // extern "C"
