// Mesh fields at arbitrary points: the evaluators through the BVH (per wave, plain and sorted), the linear scan without a BVH, the
// triangle-record kernels, the acosf self-test, their launchers, and the host path for a few points (meshEvalHostPoints).  The
// traversals themselves are mesh_distance.hpp; the sampler of the fits' rounds, mesh_sample_kernel, is fit_mesh.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>

#include "device_types.hpp"
#include "launch.hpp"
#include "mesh_distance.hpp"

namespace hpsdf {

// Mesh::SignedDistanceAtPt(pt) WITHOUT a BVH (Mesh.cpp:42-51 over the linear scan Mesh::ClosestTriangleToPt, :134-159).
// A wave takes one point and one SLICE of the triangles: lane l tests triangles first + l, first + l + 64, ... of the slice,
// keeping the first strictly smaller squared distance (so the lowest index among its own equals); the lanes fold to the
// smallest distance, ties to the lower triangle index, and the wave's winner goes into the point's 64-bit key
// (distance bits << 32 | triangle) by atomicMin -- over all slices that leaves the smallest distance and, among equals, the
// lowest triangle: what the reference's `<` scan from triangle 0 upwards keeps.  The key lives in the point's slot of the
// OUTPUT array (8 bytes, preset to all ones) -- or in scratch of the caller's when the output is host memory mapped into the
// device, where an atomic is a PCIe transaction --; mesh_naive_finish_kernel repeats the winner's closest-point test and
// writes the signed distance.  The slices let a handful of points use the whole chip (one point: 8 ms -> 0.1 ms on 1 M
// triangles); with thousands of points there is one slice and the atomic is one per wave.
// It is the checker of the BVH path on the device (TestBVHQuerying, MeshingUnitTests.cpp:110-138) and O(n) per point.
__global__ __launch_bounds__(256) void mesh_naive_kernel(MeshDev m, const double* __restrict__ xyz, size_t n, unsigned long long* __restrict__ keys,
                                                         uint32_t slices) {
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave = (point, slice), the slices of a point adjacent
    const size_t i = w / slices;
    if (i >= n) return;  // wave-uniform
    const uint32_t slice = (uint32_t)(w % slices);
    const uint32_t per = ((m.nTris + slices - 1u) / slices + 63u) & ~63u;
    const uint32_t first = slice * per, last = first + per < m.nTris ? first + per : m.nTris;
    const int lane = threadIdx.x & 63;
    const V3 pt = {(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]};
    float best = FLT_MAX;
    uint32_t bestTri = 0xFFFFFFFFu;
    const float slack = meshSlack(loadNodeUniform(m.bvh, 0));  // (the face-case tolerance of closestSimplex: the same on every path)
    for (uint32_t t = first + (uint32_t)lane; t < last; t += 64u) {
        V3 q;
        const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
        closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, best, q);
        const float d = sqnorm(pt - q);
        if (d < best) best = d, bestTri = t;
    }
    float wd = best;
    uint32_t wt = bestTri;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float od = __shfl_xor(wd, off, 64);
        const uint32_t ot = __shfl_xor(wt, off, 64);
        if (od < wd || (od == wd && ot < wt)) wd = od, wt = ot;
    }
    // (a squared distance that won a `<` against FLT_MAX is a non-negative finite float: its bits order like its value)
    if (lane == 0 && wt != 0xFFFFFFFFu) atomicMin(&keys[i], ((unsigned long long)__float_as_uint(wd) << 32) | wt);
}
__global__ __launch_bounds__(256) void mesh_naive_finish_kernel(MeshDev m, const double* __restrict__ xyz, size_t n, const unsigned long long* keys,
                                                                double* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    if (key == ~0ull) {  // no triangle came closer than FLT_MAX (a point that is not finite): the NaN of the other paths
        out[i] = (double)meshNoTriangle();
        return;
    }
    const uint32_t t = (uint32_t)key;
    const V3 pt = {(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]};
    const float slack = meshSlack(m.bvh[0]);
    V3 q;
    const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
    const int code = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, __builtin_inff(), q);
    const V3 nrm = pseudoNormal(m, t, code);
    const V3 d = pt - q;
    const float sign = dot(nrm, d) > 0.0f ? 1.0f : -1.0f;
    out[i] = (double)(sign * sqrtf(sqnorm(d)));
}

// Mesh::SignedDistanceAtPt(pt, bvh) through the traversal the sampler uses: 64 consecutive points share one walk
// (meshSignedDistanceWaveQ).  Correct for any points -- a wave visits the union of what its lanes need -- and fast when
// neighbours in the array are neighbours in space.
__global__ __launch_bounds__(256) void mesh_eval_wave_kernel(MeshDev m, const double* __restrict__ xyz, size_t n, double* __restrict__ out) {
    __shared__ MeshWaveLds sWave[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    const size_t j = active ? i : n - 1;
    const float v = meshSignedDistanceWaveQ(m, V3{(float)xyz[3 * j], (float)xyz[3 * j + 1], (float)xyz[3 * j + 2]}, active, sWave[threadIdx.x >> 6]);
    if (active) out[i] = (double)v;
}

// The same for points in ANY order: the caller's points are visited along a Morton curve over the mesh's surroundings (30-bit
// keys, an index sort), so that the 64 points of a wave are neighbours in space and share most of their walk -- 1 M random points
// of a root box: 6.9 -> 3 ms on a 2.1 M-triangle mesh; every point's value is its own, whatever the order
// (test_full_size_hierarchy_equals_linear_scan_bitwise).  Sets below kMeshEvalSortMin are not worth the sort's launches.
constexpr size_t kMeshEvalSortMin = 4096;
__device__ __forceinline__ uint32_t mortonSpread10(uint32_t v) {  // 10 bits -> every third bit
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__global__ __launch_bounds__(256) void mesh_eval_keys_kernel(MeshDev m, const double* __restrict__ xyz, uint32_t n, uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ ids) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const BvhNode& root = m.bvh[0];  // (its two child boxes: the mesh's box; a leaf root keeps the second empty)
    uint32_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool two = root.lo1[a] <= root.hi1[a];
        const float lo = two ? fminf(root.lo0[a], root.lo1[a]) : root.lo0[a], hi = two ? fmaxf(root.hi0[a], root.hi1[a]) : root.hi0[a];
        const float ext = fmaxf(hi - lo, 1e-30f);
        // the grid spans the box and as much again on either side: points of a root box around the mesh keep their order too
        const float t = ((float)xyz[3 * (size_t)i + a] - (lo - ext)) / (3.0f * ext);
        const float q = fminf(fmaxf(t, 0.0f), 1.0f) * 1023.0f;  // (NaN -> 0 through fmaxf)
        key |= mortonSpread10((uint32_t)q) << a;
    }
    keys[i] = key;
    ids[i] = i;
}
__global__ __launch_bounds__(256) void mesh_eval_wave_sorted_kernel(MeshDev m, const double* __restrict__ xyz, const uint32_t* __restrict__ ids, size_t n,
                                                                    double* __restrict__ out) {
    __shared__ MeshWaveLds sWave[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    const size_t j = ids[active ? i : n - 1];
    const float v = meshSignedDistanceWaveQ(m, V3{(float)xyz[3 * j], (float)xyz[3 * j + 1], (float)xyz[3 * j + 2]}, active, sWave[threadIdx.x >> 6]);
    if (active) out[j] = (double)v;
}

hipError_t launchMeshEvalWave(hipStream_t stream, const FieldDev& f, const double* dXyz, size_t n, double* dOut) {
    if (n == 0) return hipSuccess;
    if (f.kind != kFieldMesh || f.csgOp >= 0) return hipErrorInvalidValue;
    static const bool noSort = std::getenv("HPSDF_MESH_EVAL_NO_SORT") != nullptr;  // measurement knob
    for (size_t first = 0; first < n; first += (size_t)1 << 30) {  // a part's indices fit 32 bits
        const size_t m = std::min<size_t>((size_t)1 << 30, n - first);
        char* block = nullptr;
        size_t tmpBytes = 0;
        bool sorted = false;
        if (!noSort && m >= kMeshEvalSortMin && sortPairsU32(stream, nullptr, tmpBytes, nullptr, nullptr, nullptr, nullptr, m, 30) == hipSuccess) {
            const size_t arr = (m * sizeof(uint32_t) + 255) & ~(size_t)255;
            // stream-ordered scratch: four index arrays and the sort's own; if the pool declines, the points go as they are
            int dev = 0;
            hipMemPool_t pool = hipGetDevice(&dev) == hipSuccess ? meshPool(dev) : nullptr;  // the library's own pool, not the default one
            if (pool && hipMallocFromPoolAsync((void**)&block, 4 * arr + tmpBytes, pool, stream) == hipSuccess) {
                uint32_t *keys = (uint32_t*)block, *keysOut = (uint32_t*)(block + arr), *ids = (uint32_t*)(block + 2 * arr), *idsOut = (uint32_t*)(block + 3 * arr);
                hipLaunchKernelGGL(mesh_eval_keys_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, f.mesh, dXyz + 3 * first, (uint32_t)m, keys, ids);
                if (sortPairsU32(stream, block + 4 * arr, tmpBytes, keys, keysOut, ids, idsOut, m, 30) == hipSuccess) {
                    hipLaunchKernelGGL(mesh_eval_wave_sorted_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, f.mesh, dXyz + 3 * first, idsOut, m,
                                       dOut + first);
                    sorted = true;
                }
                (void)hipFreeAsync(block, stream);
            } else {
                (void)hipGetLastError();
            }
        }
        if (!sorted) hipLaunchKernelGGL(mesh_eval_wave_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, f.mesh, dXyz + 3 * first, m, dOut + first);
    }
    return hipGetLastError();
}

// hpsdfAcosf of the floats whose bit patterns are first, first + stride, ...: the device half of the acosf parity test
__global__ __launch_bounds__(256) void acosf_selftest_kernel(uint32_t first, uint32_t stride, size_t n, float* out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = hpsdfAcosf(__uint_as_float(first + (uint32_t)i * stride));
}
hipError_t launchAcosfSelftest(hipStream_t stream, uint32_t first, uint32_t stride, size_t n, float* dOut) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(acosf_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, first, stride, n, dOut);
    return hipGetLastError();
}

hipError_t launchMeshNaive(hipStream_t stream, const FieldDev& f, const double* dXyz, size_t n, double* dOut, unsigned long long* dKeys) {
    if (n == 0) return hipSuccess;
    if (f.kind != kFieldMesh || f.csgOp >= 0) return hipErrorInvalidValue;
    for (size_t first = 0; first < n; first += (size_t)1 << 28) {  // grid.x stays below 2^31
        const size_t m = std::min<size_t>((size_t)1 << 28, n - first);
        // enough waves to fill the chip: 256 CUs x 32 wave slots; a slice keeps at least 1024 triangles
        const uint64_t byWaves = (8192 + m - 1) / m, byTris = std::max<uint64_t>(1, f.mesh.nTris / 1024);
        const uint32_t slices = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min(byWaves, byTris), 4096));
        unsigned long long* keys = dKeys ? dKeys + first : reinterpret_cast<unsigned long long*>(dOut + first);
        hipError_t e = hipMemsetAsync(keys, 0xFF, m * sizeof(double), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(mesh_naive_kernel, dim3((unsigned)((m * slices + 3) / 4)), dim3(256), 0, stream, f.mesh, dXyz + 3 * first, m, keys, slices);
        hipLaunchKernelGGL(mesh_naive_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, f.mesh, dXyz + 3 * first, m, keys,
                           dOut + first);
    }
    return hipGetLastError();
}

// MeshDev::triPos: per triangle one 48-byte record -- the nine vertex coordinates and the unnormalised normal
// cross(b - a, c - a) -- gathered once per mesh: a closest-point test is three 16-byte loads instead of index -> vertex chains
__global__ __launch_bounds__(256) void mesh_tripos_kernel(const float* __restrict__ verts, const uint32_t* __restrict__ tris,
                                                          uint64_t nTris, float4* __restrict__ triPos) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nTris) return;
    const uint32_t ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
    const V3 a = {verts[3 * (size_t)ia], verts[3 * (size_t)ia + 1], verts[3 * (size_t)ia + 2]};
    const V3 b = {verts[3 * (size_t)ib], verts[3 * (size_t)ib + 1], verts[3 * (size_t)ib + 2]};
    const V3 c = {verts[3 * (size_t)ic], verts[3 * (size_t)ic + 1], verts[3 * (size_t)ic + 2]};
    const V3 n = cross(b - a, c - a);
    triPos[3 * t] = make_float4(a.x, a.y, a.z, b.x);
    triPos[3 * t + 1] = make_float4(b.y, b.z, c.x, c.y);
    triPos[3 * t + 2] = make_float4(c.z, n.x, n.y, n.z);
}

// MeshDev::triPre: per leaf slot the data of the lower-bound test (triLowerBound2) and the triangle's index: the unit normal n,
// a unit vector u along the longest edge, the centre g of the triangle's bounding rectangle in the (u, n x u) frame and the
// rectangle's half-extents.  The bound is valid for ANY orthonormal n, u as long as every point x of the triangle has
// |n . (x - g)| <= e, |u . (x - g)| <= hu and sqrt(|x - g|^2 - (n . (x - g))^2 - (u . (x - g))^2) <= hv -- all three are convex in x,
// so the vertices decide, and all three are MEASURED here against the g that is stored, with the arithmetic of the test.  When e
// is not negligible (slivers, whose cross product cancels) or the frame is not orthonormal to 1e-6, n and u are set to zero and hv
// to the largest distance of a vertex from g, which turns the test into the ball's bound |p - g| - rho.  What is left of e
// (<= 4e-7 of the mesh's scale) and of the frame's rounding is covered by the caller's slack (2e-6 of that scale: meshSlack).
__global__ __launch_bounds__(256) void mesh_tripre_kernel(const float* __restrict__ verts, const uint32_t* __restrict__ tris,
                                                          const uint32_t* __restrict__ slotTri, uint64_t nTris, float4* __restrict__ triPre) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nTris) return;
    const uint32_t t = slotTri ? slotTri[s] : (uint32_t)s;
    const uint32_t ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2];
    const V3 a = {verts[3 * (size_t)ia], verts[3 * (size_t)ia + 1], verts[3 * (size_t)ia + 2]};
    const V3 b = {verts[3 * (size_t)ib], verts[3 * (size_t)ib + 1], verts[3 * (size_t)ib + 2]};
    const V3 c = {verts[3 * (size_t)ic], verts[3 * (size_t)ic + 1], verts[3 * (size_t)ic + 2]};
    const V3 ab = b - a, ac = c - a, bc = c - b;
    const float lab = sqnorm(ab), lac = sqnorm(ac), lbc = sqnorm(bc);
    const V3 n = cross(ab, ac);
    const float inf = __builtin_inff();
    // the frame: n, u along the longest edge, v = n x u; the rectangle's centre from the vertices' (u, v) ranges about a
    const V3 le = lab >= lac && lab >= lbc ? ab : (lac >= lbc ? ac : bc);
    const float len = sqrtf(sqnorm(n)), ll = sqrtf(sqnorm(le));
    V3 nh = {0.0f, 0.0f, 0.0f}, uh = {0.0f, 0.0f, 0.0f};
    const float third = 1.0f / 3.0f;
    V3 g = third * (a + (b + c));
    bool framed = len > 0.0f && len < inf && ll > 0.0f && ll < inf;
    if (framed) {
        nh = (1.0f / len) * n;
        uh = (1.0f / ll) * le;
        const V3 vh = cross(nh, uh);
        const float ub = dot(uh, ab), uc = dot(uh, ac), vb = dot(vh, ab), vc = dot(vh, ac);  // (vertex a sits at (0, 0))
        const float um = 0.5f * (fminf(0.0f, fminf(ub, uc)) + fmaxf(0.0f, fmaxf(ub, uc)));
        const float vm = 0.5f * (fminf(0.0f, fminf(vb, vc)) + fmaxf(0.0f, fmaxf(vb, vc)));
        g = a + (um * uh + vm * vh);
        framed = fabsf(sqnorm(nh) - 1.0f) <= 1e-6f && fabsf(sqnorm(uh) - 1.0f) <= 1e-6f && fabsf(dot(nh, uh)) <= 1e-6f;
    }
    const V3 da = a - g, db = b - g, dc = c - g;
    const float ra = sqnorm(da), rb = sqnorm(db), rcq = sqnorm(dc);
    const float rho = sqrtf(fmaxf(ra, fmaxf(rb, rcq))) * 1.00001f + 1e-30f;
    // the scale the caller's slack is proportional to is at least this (the mesh's extent or its largest coordinate)
    const float scale = fmaxf(rho, fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fabsf(g.z)));
    float hu = 0.0f, hv = rho;
    if (framed) {
        const float sa = dot(nh, da), sb = dot(nh, db), sc = dot(nh, dc);
        const float ua = dot(uh, da), ub = dot(uh, db), uc = dot(uh, dc);
        const float e = fmaxf(fabsf(sa), fmaxf(fabsf(sb), fabsf(sc)));
        const float wa = sqrtf(fmaxf(ra - sa * sa - ua * ua, 0.0f)), wb = sqrtf(fmaxf(rb - sb * sb - ub * ub, 0.0f)),
                    wc = sqrtf(fmaxf(rcq - sc * sc - uc * uc, 0.0f));
        // The rectangle holds the TRIANGLE (measured above, with allowances for its own rounding).  What the closest-point routine
        // returns for the triangle lies within a quarter of the traversal's slack of it: closestSimplex does not take a face-case
        // point farther outside than that (until round 4 the rectangle was widened by a "play" of 1e-6 longest edge / sin(smallest
        // angle) instead, an estimate of how far the reference's barycentric quotients can throw q: it did not hold on needles).
        hu = fmaxf(fabsf(ua), fmaxf(fabsf(ub), fabsf(uc))) * 1.00001f + 4e-7f * scale;
        // (hv also takes 1e-3 hu: the test forms the in-plane distance across u as sqrt(|d|^2 - s^2 - a^2), whose cancellation leaves up to
        // sqrt(2 ulp) |d| = 3.5e-4 |d| where the true value is nearly zero -- beside a needle that is more than its width; past ~3 hu from
        // g the excess is below 1e-6 of the bound itself, which rejectBound's factor covers)
        hv = fmaxf(wa, fmaxf(wb, wc)) * 1.00001f + 4e-7f * scale + 1e-3f * hu;
        framed = e <= 4e-7f * scale && hu < inf && hv < inf;
    }
    if (!framed || !(rho < inf)) {  // (non-finite input: the bound degenerates to "always passes" via NaN)
        nh = V3{0.0f, 0.0f, 0.0f}, uh = V3{0.0f, 0.0f, 0.0f};
        hu = 0.0f, hv = rho;
    }
    triPre[3 * s] = make_float4(g.x, g.y, g.z, hu);
    triPre[3 * s + 1] = make_float4(nh.x, nh.y, nh.z, hv);
    triPre[3 * s + 2] = make_float4(uh.x, uh.y, uh.z, __uint_as_float(t));
}

hipError_t launchMeshTriPos(hipStream_t stream, const float* dVerts, const uint32_t* dTris, uint64_t nTris, float* dTriPos,
                            const uint32_t* dSlotTri, float* dTriPre) {
    if (nTris == 0) return hipSuccess;
    if (dTriPos)
        hipLaunchKernelGGL(mesh_tripos_kernel, dim3((unsigned)((nTris + 255) / 256)), dim3(256), 0, stream, dVerts, dTris, nTris,
                           reinterpret_cast<float4*>(dTriPos));
    if (dTriPre)
        hipLaunchKernelGGL(mesh_tripre_kernel, dim3((unsigned)((nTris + 255) / 256)), dim3(256), 0, stream, dVerts, dTris, dSlotTri, nTris,
                           reinterpret_cast<float4*>(dTriPre));
    return hipGetLastError();
}

// Mesh::SignedDistanceAtPt(pt, bvh) for a few points, on the calling thread: `hm` holds HOST copies of the field's arrays (capi_field.cpp
// keeps them with the field after the first such call).  The per-point stack traversal of meshSignedDistance, compiled for the host
// from the very statements the device runs: the same bits as every device path (tests/test_gpu_parity.py).
void meshEvalHostPoints(const MeshDev& hm, const double* xyz, size_t n, double* out) {
    // The previous answer of this thread is tried first (the `hint` of meshSignedDistance: a search that starts with a tight bound visits
    // a fraction of the nodes; the answer does not depend on it).  Successive one-point calls of a thread are what a per-sample SDF lambda
    // makes: neighbouring samples of one cell.
    static thread_local uint32_t hint = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i)
        out[i] = (double)meshSignedDistance(hm, V3{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]}, hint);
}

}  // namespace hpsdf
