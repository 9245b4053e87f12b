// hpsdf_extract_surface_dual: dual contouring over the lattice of hpsdf_extract_surface (no reference counterpart; include/hpsdf.h
// states the samples, the vertex and the ordering; the vertex's statements are dual_vertex.hpp's).
//
//   1. lattice_query_kernel (kernels.hip): every lattice value, as the dense marching-cubes call;
//   2. dual_edge_words_kernel: one wave per 64 edge ids -- two ballots, the crossing edges and the interior crossing edges, each a
//      word and its popcount;  dual_cube_words_kernel: one wave per 64 cubes, the ballot of the mixed cubes;  three rocprim
//      exclusive scans of the counts (64-bit);
//   3. dual_hermite_kernel<MAXP>: one lane a crossing edge, found through the words as surf_vertex_kernel finds it: the edge's vertex
//      (edgeVertex) through trueGradientPoint, into the 64-byte record at the edge's prefix + rank;
//   4. dual_cube_list_kernel writes the list of mixed cubes from the cube words;  dual_vertex_kernel runs one lane a LISTED cube (full
//      waves): each of the cube's up to 12 records is looked up by word prefix + popcount, as surf_tri_kernel looks up a vertex, once
//      for the mean and once for the normal equations, which are then solved and the vertex and its info byte written;
//   5. dual_quad_kernel: one lane a crossing edge; an interior one looks up its four cubes' vertex ids through the cube words'
//      prefixes and writes two triangles at 2 x its interior rank.
// No atomics: every output position is a prefix, so the output is deterministic.  Scratch (one allocation, freed before returning):
// values 8 B a point, per 64 edge ids 2 x (8 + 4 + 8) B, per 64 cubes 20 B, the scans' temporary storage; then the outputs' allocation:
// 64 B a crossing edge, 4 + 24 + 1 B a mixed cube, 24 B a triangle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "device_types.hpp"
#include "dual_vertex.hpp"
#include "jet_point.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "surface_common.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kDualMaxGrid = 8192;

struct DualArgs {
    SurfaceLattice g;
    double iso, tau;
    uint64_t nEdges;  // 3 nPts
    uint64_t nWords;  // ceil(nEdges / 64)
    uint64_t nCubes;
    uint64_t nTiles;  // ceil(nCubes / 64)
};

__device__ __forceinline__ uint64_t bitsBelow(uint32_t bit) { return (1ull << bit) - 1ull; }

// edge id -> its lower point L, axis and the point's indices
__device__ __forceinline__ void edgeOf(const DualArgs& A, uint64_t e, uint32_t& L, uint32_t& a, uint32_t (&idx)[3]) {
    L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
    idx[0] = L % A.g.np[0], idx[1] = (L / A.g.np[0]) % A.g.np[1], idx[2] = (L / A.g.np[0]) / A.g.np[1];
}
__device__ __forceinline__ uint32_t strideOf(const DualArgs& A, uint32_t a) { return a == 0 ? 1u : (a == 1 ? A.g.np[0] : A.g.np[0] * A.g.np[1]); }

__global__ __launch_bounds__(kSurfThreads) void dual_edge_words_kernel(const double* __restrict__ v, DualArgs A, uint64_t* __restrict__ eWords,
                                                                     uint32_t* __restrict__ eCounts, uint64_t* __restrict__ iWords,
                                                                     uint32_t* __restrict__ iCounts) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; e < total; e += stride) {  // wave-uniform: total is whole waves
        bool crosses = false, interior = false;
        if (e < A.nEdges) {
            uint32_t L, a, idx[3];
            edgeOf(A, e, L, a, idx);
            if (idx[a] < A.g.n[a]) {  // (otherwise the edge would leave the lattice)
                crosses = (v[L] < A.iso) != (v[L + strideOf(A, a)] < A.iso);
                interior = crosses && dualInterior(idx, a, A.g.n);
            }
        }
        const uint64_t em = __ballot(crosses), im = __ballot(interior);
        if ((threadIdx.x & 63u) == 0) {
            eWords[e >> 6] = em, eCounts[e >> 6] = (uint32_t)__popcll(em);
            iWords[e >> 6] = im, iCounts[e >> 6] = (uint32_t)__popcll(im);
        }
    }
}

// lower corner's lattice point of cube q
__device__ __forceinline__ uint32_t cubeBase(const DualArgs& A, uint32_t Q, uint32_t (&idx)[3]) {
    idx[0] = Q % A.g.n[0], idx[1] = (Q / A.g.n[0]) % A.g.n[1], idx[2] = (Q / A.g.n[0]) / A.g.n[1];
    return idx[0] + A.g.np[0] * (idx[1] + A.g.np[1] * idx[2]);
}

__global__ __launch_bounds__(kSurfThreads) void dual_cube_words_kernel(const double* __restrict__ v, DualArgs A, uint64_t* __restrict__ cWords,
                                                                     uint32_t* __restrict__ cCounts) {
    const uint32_t sy = A.g.np[0], sz = A.g.np[0] * A.g.np[1];
    const uint32_t off[8] = {0u, 1u, sy, sy + 1u, sz, sz + 1u, sz + sy, sz + sy + 1u};
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; q < total; q += stride) {
        bool mixed = false;
        if (q < A.nCubes) {
            uint32_t idx[3];
            const uint32_t L0 = cubeBase(A, (uint32_t)q, idx);
            uint32_t c = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) c |= (v[L0 + off[b]] < A.iso ? 1u : 0u) << b;
            mixed = c != 0u && c != 255u;
        }
        const uint64_t m = __ballot(mixed);
        if ((threadIdx.x & 63u) == 0) cWords[q >> 6] = m, cCounts[q >> 6] = (uint32_t)__popcll(m);
    }
}

template <int MAXP>
__global__ __launch_bounds__(kSurfThreads) void dual_hermite_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ v,
                                                                  DualArgs A, const uint64_t* __restrict__ eWords,
                                                                  const uint64_t* __restrict__ ePrefix, DualRecord* __restrict__ recs) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; e < total; e += stride) {
        const uint64_t word = eWords[e >> 6];  // (one address for the whole wave)
        if (word == 0) continue;               // wave-uniform
        const uint32_t lane = (uint32_t)(e & 63u);
        if (!((word >> lane) & 1u)) continue;
        const uint64_t id = ePrefix[e >> 6] + (uint64_t)__popcll(word & bitsBelow(lane));
        uint32_t L, a, idx[3];
        edgeOf(A, e, L, a, idx);
        double p[3], g[3];
        edgeVertex(A.g.lo, A.g.h, idx, a, v[L], v[L + strideOf(A, a)], A.iso, p);
        const double f = trueGradientPoint<MAXP>(t, p[0], p[1], p[2], false, sNl, sRec, g);
        DualRecord& r = recs[id];
        r.p[0] = p[0], r.p[1] = p[1], r.p[2] = p[2], r.f = f;
        r.g[0] = g[0], r.g[1] = g[1], r.g[2] = g[2], r.pad = 0.0;
    }
}

__global__ __launch_bounds__(kSurfThreads) void dual_cube_list_kernel(DualArgs A, const uint64_t* __restrict__ cWords,
                                                                    const uint64_t* __restrict__ cPrefix, uint32_t* __restrict__ list) {
    const uint64_t total = A.nTiles * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; q < total; q += stride) {
        const uint64_t word = cWords[q >> 6];
        const uint32_t lane = (uint32_t)(q & 63u);
        if ((word >> lane) & 1u) list[cPrefix[q >> 6] + (uint64_t)__popcll(word & bitsBelow(lane))] = (uint32_t)q;
    }
}

__global__ __launch_bounds__(kSurfThreads) void dual_vertex_kernel(DualArgs A, int leftAssoc, const uint32_t* __restrict__ list, uint64_t nVerts,
                                                                 const uint64_t* __restrict__ eWords, const uint64_t* __restrict__ ePrefix,
                                                                 const DualRecord* __restrict__ recs, double* __restrict__ verts,
                                                                 uint8_t* __restrict__ info) {
    const uint32_t sy = A.g.np[0], sz = A.g.np[0] * A.g.np[1];
    const uint32_t cornerOff[8] = {0u, 1u, sy, sy + 1u, sz, sz + 1u, sz + sy, sz + sy + 1u};
    const uint64_t stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t vtx = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; vtx < nVerts; vtx += stride) {
        uint32_t idx[3];
        const uint32_t L0 = cubeBase(A, list[vtx], idx);
        // pass 1: which of the 12 edges cross, their records, the mean of their points
        uint32_t rid[12], k = 0, crossing = 0;
        DualNormal N;
        double sum[3], m[3];
        dualClear(N, sum);
#pragma unroll
        for (uint32_t e = 0; e < 12u; ++e) {
            const uint64_t ge = 3u * (uint64_t)(L0 + cornerOff[dualEdgeCorner(e)]) + dualEdgeAxis(e);
            const uint64_t w = eWords[ge >> 6];
            const uint32_t bit = (uint32_t)(ge & 63u);
            rid[e] = 0;
            if ((w >> bit) & 1u) {
                rid[e] = (uint32_t)(ePrefix[ge >> 6] + (uint64_t)__popcll(w & bitsBelow(bit)));
                crossing |= 1u << e;
                ++k;
                dualAddPoint(recs[rid[e]].p, sum);
            }
        }
        dualMean(sum, k, m);  // (a listed cube is mixed: k >= 3)
        // pass 2: the normal equations, one record at a time
#pragma unroll
        for (uint32_t e = 0; e < 12u; ++e) {
            if (!((crossing >> e) & 1u)) continue;
            const DualRecord r = recs[rid[e]];
            dualAccumulate(r.p, r.f, r.g, m, A.iso, leftAssoc, N);
        }
        double cubeLo[3], cubeHi[3], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            cubeLo[a] = A.g.lo[a] + (double)idx[a] * A.g.h[a];
            cubeHi[a] = A.g.lo[a] + (double)(idx[a] + 1u) * A.g.h[a];
        }
        const uint32_t inf = dualSolve(N, m, A.tau, leftAssoc, cubeLo, cubeHi, x);
        verts[3 * vtx] = x[0], verts[3 * vtx + 1] = x[1], verts[3 * vtx + 2] = x[2];
        info[vtx] = (uint8_t)inf;
    }
}

__global__ __launch_bounds__(kSurfThreads) void dual_quad_kernel(const double* __restrict__ v, DualArgs A, const uint64_t* __restrict__ iWords,
                                                               const uint64_t* __restrict__ iPrefix, const uint64_t* __restrict__ cWords,
                                                               const uint64_t* __restrict__ cPrefix, uint64_t* __restrict__ tris) {
    const uint64_t total = A.nWords * 64u, stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; e < total; e += stride) {
        const uint64_t word = iWords[e >> 6];
        if (word == 0) continue;  // wave-uniform
        const uint32_t lane = (uint32_t)(e & 63u);
        if (!((word >> lane) & 1u)) continue;
        const uint64_t first = 2u * (iPrefix[e >> 6] + (uint64_t)__popcll(word & bitsBelow(lane)));
        uint32_t L, a, idx[3], Q[4];
        edgeOf(A, e, L, a, idx);
        dualQuadCubes(idx, a, A.g.n, Q);
        uint64_t q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = cPrefix[Q[c] >> 6] + (uint64_t)__popcll(cWords[Q[c] >> 6] & bitsBelow(Q[c] & 63u));
        if (!(v[L] < A.iso)) {  // the lower end is outside: the quad is reversed
            const uint64_t s = q[1];
            q[1] = q[3], q[3] = s;
        }
        uint64_t* o = tris + 3 * first;
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        o[3] = q[0], o[4] = q[2], o[5] = q[3];
    }
}

// per-phase device times of this thread's last call (hpsdf_surface_dual_last_timings), from events on the context stream
thread_local double tDualMs[8] = {0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

}  // namespace hpsdf

using namespace hpsdf;

extern "C" {

int hpsdf_surface_dual_last_timings(double* ms) {
    if (!ms) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    std::memcpy(ms, tDualMs, sizeof tDualMs);
    return HPSDF_OK;
}

int hpsdf_extract_surface_dual(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3], double iso,
                               double tau, uint32_t flags, double** verts, uint64_t* nVerts, uint64_t** tris, uint64_t* nTris,
                               uint8_t** vertInfo, double* values) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || !lo || !hi || !n || !verts || !nVerts || !tris || !nTris) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *verts = nullptr, *tris = nullptr, *nVerts = 0, *nTris = 0;
    if (vertInfo) *vertInfo = nullptr;
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    static const char* kWhat = "hpsdf_extract_surface_dual";
    if (const int rc = dualArgumentError(tau, flags)) return rc;
    CheckedLattice cl{};
    if (const int rc = checkLattice(kWhat, kDenseLimits, t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, iso, &cl)) return rc;
    const uint64_t nPts = cl.nPts;
    DualArgs A{};
    SurfaceLattice& g = A.g;
    for (int a = 0; a < 3; ++a) g.lo[a] = cl.lo[a], g.h[a] = cl.h[a], g.n[a] = cl.n[a], g.np[a] = cl.n[a] + 1u;
    g.nPts = (uint32_t)nPts;
    A.iso = iso, A.tau = tau;
    A.nEdges = 3 * nPts;
    A.nWords = (A.nEdges + 63) / 64;
    A.nCubes = cl.nCubes;
    A.nTiles = (cl.nCubes + 63) / 64;
    const uint64_t nW = A.nWords, nT = A.nTiles;

    HPSDF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // scratch, one allocation: values | edge words, interior words, cube words | their counts | their prefixes | scan storage
    size_t tmpW = 0, tmpT = 0;
    if (const int rc = primStatus(prefixScan(nullptr, nullptr, nW + 1, s)(nullptr, tmpW), kPrefixScan)) return rc;
    if (const int rc = primStatus(prefixScan(nullptr, nullptr, nT + 1, s)(nullptr, tmpT), kPrefixScan)) return rc;
    const size_t oVals = 0, oEw = alignUp(oVals + nPts * 8), oIw = alignUp(oEw + nW * 8), oCw = alignUp(oIw + nW * 8),
                 oEc = alignUp(oCw + nT * 8), oIc = alignUp(oEc + (nW + 1) * 4), oCc = alignUp(oIc + (nW + 1) * 4),
                 oEp = alignUp(oCc + (nT + 1) * 4), oIp = alignUp(oEp + (nW + 1) * 8), oCp = alignUp(oIp + (nW + 1) * 8),
                 oTmp = alignUp(oCp + (nT + 1) * 8), total = oTmp + std::max(tmpW, tmpT) + 256;
    DevPool pool(kWhat);
    char* base = nullptr;
    SURF_ALLOC(pool, base, total, "scratch");
    double* dV = (double*)(base + oVals);
    uint64_t *dEw = (uint64_t*)(base + oEw), *dIw = (uint64_t*)(base + oIw), *dCw = (uint64_t*)(base + oCw);
    uint32_t *dEc = (uint32_t*)(base + oEc), *dIc = (uint32_t*)(base + oIc), *dCc = (uint32_t*)(base + oCc);
    uint64_t *dEp = (uint64_t*)(base + oEp), *dIp = (uint64_t*)(base + oIp), *dCp = (uint64_t*)(base + oCp);
    void* dTmp = base + oTmp;

    for (double& x : tDualMs) x = 0.0;
    Events<9> ev;
    TreeDev td = t->dev;
    td.leftAssoc = reductionLeftAssoc(ctx);
    const dim3 block(kSurfThreads), edgeGrid(gridOf(nW * 64, kDualMaxGrid)), cubeGrid(gridOf(nT * 64, kDualMaxGrid));
    ev.mark(0, s);
    HPSDF_HIP(launchQueryLattice(s, td, ctx->dTables, A.g, dV));
    ev.mark(1, s);
    HPSDF_HIP(hipMemsetAsync(dEc + nW, 0, 4, s));
    HPSDF_HIP(hipMemsetAsync(dIc + nW, 0, 4, s));
    HPSDF_HIP(hipMemsetAsync(dCc + nT, 0, 4, s));
    hipLaunchKernelGGL(dual_edge_words_kernel, edgeGrid, block, 0, s, dV, A, dEw, dEc, dIw, dIc);
    HPSDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(dual_cube_words_kernel, cubeGrid, block, 0, s, dV, A, dCw, dCc);
    HPSDF_HIP(hipGetLastError());
    ev.mark(2, s);
    if (const int rc = primStatus(prefixScan(dEc, dEp, nW + 1, s)(dTmp, tmpW), kPrefixScan)) return rc;
    if (const int rc = primStatus(prefixScan(dIc, dIp, nW + 1, s)(dTmp, tmpW), kPrefixScan)) return rc;
    if (const int rc = primStatus(prefixScan(dCc, dCp, nT + 1, s)(dTmp, tmpT), kPrefixScan)) return rc;
    ev.mark(3, s);
    uint64_t counts[3] = {0, 0, 0};
    HPSDF_HIP(hipMemcpyAsync(&counts[0], dEp + nW, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipMemcpyAsync(&counts[1], dIp + nW, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipMemcpyAsync(&counts[2], dCp + nT, 8, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipStreamSynchronize(s));
    const uint64_t E = counts[0], V = counts[2], T = 2 * counts[1];

    HostOut hVerts, hTris, hInfo;
    if (V > 0) {
        hVerts.p = std::malloc(V * 3 * sizeof(double));
        if (T > 0) hTris.p = std::malloc(T * 3 * sizeof(uint64_t));
        if (vertInfo) hInfo.p = std::malloc(V);
        if (!hVerts.p || (T > 0 && !hTris.p) || (vertInfo && !hInfo.p))
            return fail(HPSDF_ERR_OUT_OF_MEMORY, std::string(kWhat) + ": host allocation failed");
        // the outputs' allocation: records | cube list | vertices | triangles | info bytes
        const size_t oList = alignUp(E * sizeof(DualRecord)), oVerts = alignUp(oList + V * 4), oTris = alignUp(oVerts + V * 24),
                     oInfo = alignUp(oTris + T * 24);
        char* outs = nullptr;
        SURF_ALLOC(pool, outs, oInfo + V, "records and outputs");
        DualRecord* dRecs = (DualRecord*)outs;
        uint32_t* dList = (uint32_t*)(outs + oList);
        double* dVerts = (double*)(outs + oVerts);
        uint64_t* dTris = (uint64_t*)(outs + oTris);
        uint8_t* dInfo = (uint8_t*)(outs + oInfo);
        ev.mark(4, s);
        forMaxDegree<2, 3, 5, 12>(td.maxDegree, [&](auto P) {
            hipLaunchKernelGGL((dual_hermite_kernel<decltype(P)::value>), edgeGrid, block, 0, s, td, ctx->dTables, dV, A, dEw, dEp, dRecs);
        });
        HPSDF_HIP(hipGetLastError());
        ev.mark(5, s);
        hipLaunchKernelGGL(dual_cube_list_kernel, cubeGrid, block, 0, s, A, dCw, dCp, dList);
        HPSDF_HIP(hipGetLastError());
        hipLaunchKernelGGL(dual_vertex_kernel, dim3(gridOf(V, kDualMaxGrid)), block, 0, s, A, (int)td.leftAssoc, dList, V, dEw, dEp, dRecs, dVerts,
                           dInfo);
        HPSDF_HIP(hipGetLastError());
        ev.mark(6, s);
        if (T > 0) {
            hipLaunchKernelGGL(dual_quad_kernel, edgeGrid, block, 0, s, dV, A, dIw, dIp, dCw, dCp, dTris);
            HPSDF_HIP(hipGetLastError());
        }
        ev.mark(7, s);
        HPSDF_HIP(hipMemcpyAsync(hVerts.p, dVerts, V * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        if (T > 0) HPSDF_HIP(hipMemcpyAsync(hTris.p, dTris, T * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (vertInfo) HPSDF_HIP(hipMemcpyAsync(hInfo.p, dInfo, V, hipMemcpyDeviceToHost, s));
    }
    if (values) HPSDF_HIP(hipMemcpyAsync(values, dV, nPts * sizeof(double), hipMemcpyDeviceToHost, s));
    ev.mark(8, s);
    HPSDF_HIP(hipStreamSynchronize(s));
    tDualMs[0] = ev.ms(0, 1), tDualMs[1] = ev.ms(1, 2), tDualMs[2] = ev.ms(2, 3);
    if (V > 0) tDualMs[3] = ev.ms(4, 5), tDualMs[4] = ev.ms(5, 6), tDualMs[5] = ev.ms(6, 7);
    tDualMs[6] = ev.ms(V > 0 ? 7 : 3, 8);
    tDualMs[7] = ev.ms(0, 8);
    if (V > 0) {
        *verts = (double*)hVerts.p, *tris = (uint64_t*)hTris.p;
        if (vertInfo) *vertInfo = (uint8_t*)hInfo.p;
        hVerts.p = hTris.p = hInfo.p = nullptr;
        *nVerts = V, *nTris = T;
    }
    return HPSDF_OK;
    HPSDF_CATCH
}

}  // extern "C"
