// The bit-exact fit kernels of fit_kernels.hpp for fields of kind kFieldMesh (32 fit_kernel, 4 fit_multi_kernel, 4 field_kernel), and
// the first half of a mesh round, mesh_sample_kernel with its launchers.  The sampler sits here and not with the other mesh kernels
// (mesh_field.hip) because it shares meshSampleOrder with fitBlockBody: compiled without that second caller the compiler
// specialises the function for the sampler's arguments and mesh_sample_kernel comes out with a different instruction stream.
#include <cstdlib>

#include "fit_kernels.hpp"

namespace hpsdf {

// Mesh fields, first half of a round: F at every sample of every fit, written where fit_kernel<kFieldSamples> reads it
// (FitTask::sampleOff + (i nq + j) nq + k).  A closest-triangle traversal costs anything between a few dozen and tens
// of thousands of steps depending on where the cell lies, so sampling inside the fit kernel (one workgroup per cell)
// left the chip a quarter full behind the expensive cells; here the unit of work is one wave = 64 samples that sit
// next to each other (meshSampleOrder over the whole grid), a workgroup is four of them, the hardware deals them out,
// and without the fit's accumulators twice as many waves fit on a CU.  grid = (ceil(nq^3 / 256), tasks of one degree).
// range == nullptr: grid = (chunks of 256 samples, tasks).  Otherwise grid.y is an upper bound and row y samples task
// range[0] + y if y < range[1] -- the device-side frontier's rounds (frontier.hip), whose task counts the host does not know.
#ifndef HPSDF_MESH_WG
#define HPSDF_MESH_WG 64  // threads of a sampling workgroup (a multiple of 64): the hardware deals out workgroups, so this is the grain of its load balancing
#endif
constexpr int kMeshWg = HPSDF_MESH_WG;
constexpr uint32_t kMeshXcdRun = 128;  // workgroups of 64 samples: runs of 64-256 measure alike; 1 (plain order) and >= 1024 lose 3-7 %
static uint32_t meshXcdRun() {  // HPSDF_MESH_XCD_RUN overrides (experiments); 1 = plain dispatch order
    static const uint32_t v = [] {
        const char* e = std::getenv("HPSDF_MESH_XCD_RUN");
        const long x = e ? std::atol(e) : (long)kMeshXcdRun;
        return (uint32_t)(x < 1 ? 1 : (x > 4096 ? 4096 : x));
    }();
    return v;
}
#ifndef HPSDF_MESH_MIN_WAVES
#define HPSDF_MESH_MIN_WAVES 6  // <= 80 registers, six waves a SIMD (round 6; 88 registers and five waves until then: the kernel is bound by instruction issue with a third of the slots empty, and a sixth wave fills some of them -- Create on the 2.1 M-triangle torus at 1e-6 32.1 -> 30.7 ms, 1.3 M-triangle icosphere 11.4 -> 10.9, at the price of 48 more bytes of scratch)
#endif
__global__ __launch_bounds__(kMeshWg, HPSDF_MESH_MIN_WAVES) void mesh_sample_kernel(const FitTask* __restrict__ tasks, int degree,
                                                          const DeviceTables* __restrict__ T, MeshDev mesh, RootMap rm,
                                                          double* __restrict__ samples, const uint32_t* __restrict__ range,
                                                          uint32_t nTasksArg, uint32_t xcdRun) {
    __shared__ MeshWaveLds sWave[kMeshWg / 64];
    __shared__ double sR[64];
    __shared__ unsigned char sPos[64];
    // Which (task, chunk) this workgroup samples.  Workgroups are dealt round-robin over the 8 XCDs in dispatch order
    // (blocks b and b + 8 share an XCD and its 4 MB L2: MI355X_MICROARCH.md, observed, a speed matter only), and the
    // tasks lie in node order, i.e. along the octree's space-filling curve.  The (task, chunk) list is cut into runs of
    // kMeshXcdRun consecutive entries -- a few neighbouring cells -- and the runs are dealt round-robin over the XCDs:
    // what an XCD has in flight at any time is a handful of compact regions, whose part of the BVH and of the triangle
    // records is all its L2 has to hold (plain blockIdx order: every eighth chunk of an eight times longer stretch;
    // one contiguous eighth of the list per XCD instead keeps the locality but not the balance -- cells far from the
    // surface cost several times more than cells on it).
    const uint32_t gx = gridDim.x, nTasks = range != nullptr ? range[1] : nTasksArg;
    const uint32_t nwg = nTasks * gx, orig = blockIdx.y * gx + blockIdx.x;
    const uint32_t inXcd = orig >> 3;  // position in the sequence of the workgroups that share this one's XCD
    const uint32_t wgid = (((inXcd / xcdRun) << 3) + (orig & 7u)) * xcdRun + inXcd % xcdRun;
    if (wgid >= nwg) return;  // (the grid is rounded up to whole groups of 8 runs, or an upper bound)
    const uint32_t chunk = wgid % gx;
    uint32_t task = wgid / gx;
    if (range != nullptr) task += range[0];
    const int tid = threadIdx.x, nq = 4 * degree + 1, gl = nq * (nq - 1) / 2, total = nq * nq * nq;
    if (tid < nq) sR[tid] = T->roots[gl + tid];
    __syncthreads();
    if (tid < nq) {
        int rank = 0;
        for (int b = 0; b < nq; ++b) rank += sR[b] < sR[tid] ? 1 : 0;
        sPos[rank] = (unsigned char)tid;
    }
    __syncthreads();
    const FitTask& tk = tasks[task];
    const int r = (int)chunk * kMeshWg + tid;
    const bool active = r < total;
    const int rem = meshSampleOrder(active ? r : total - 1, nq, nq, sPos, sPos);
    const int i = rem / (nq * nq), jk = rem - i * nq * nq, j = jk / nq, k = jk - j * nq;
    double w[3];
    const int idx[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double sc = (double)(tk.bmax[a] - tk.bmin[a]) * 0.5;       // Octree.cpp:1020 sizes() in f32
        const double ce = (double)((tk.bmin[a] + tk.bmax[a]) / 2.0f);     // :1021 center() in f32
        const double u = sR[idx[a]] * sc + ce;                            // :1035-1037
        w[a] = u * rm.bounds[a] + rm.centre[a];                           // :327
    }
    const float mv = meshSignedDistanceWaveQ(mesh, V3{(float)w[0], (float)w[1], (float)w[2]}, active, sWave[tid >> 6]);
    if (active) samples[tk.sampleOff + (uint64_t)rem] = (double)mv;
}

hipError_t launchMeshSample(hipStream_t stream, const FitTask* dTasks, uint32_t nTasks, int degree, const DeviceTables* dTables,
                            const FieldDev& field, const RootMap& rm, double* dSamples) {
    if (nTasks == 0) return hipSuccess;
    if (degree < 1 || degree > 12 || field.kind != kFieldMesh) return hipErrorInvalidValue;
    const int nq = 4 * degree + 1;
    const unsigned gx = (unsigned)((nq * nq * nq + kMeshWg - 1) / kMeshWg);
    for (uint32_t first = 0; first < nTasks; first += 65535u) {
        const uint32_t n = nTasks - first < 65535u ? nTasks - first : 65535u;
        // (grid rounded up to whole groups of 8 runs of the XCD interleave)
        const uint32_t run = meshXcdRun(), wgs = (n * gx + 8u * run - 1u) / (8u * run) * (8u * run);
        hipLaunchKernelGGL(mesh_sample_kernel, dim3(gx, (wgs + gx - 1u) / gx), dim3(kMeshWg), 0, stream, dTasks + first, degree, dTables, field.mesh, rm,
                           dSamples, (const uint32_t*)nullptr, n, run);
    }
    return hipGetLastError();
}

// the same over the device-written task range dRange = {first task, count} of dTasks; maxTasks bounds the count
hipError_t launchMeshSampleRange(hipStream_t stream, const FitTask* dTasks, const uint32_t* dRange, uint32_t maxTasks, int degree,
                                 const DeviceTables* dTables, const FieldDev& field, const RootMap& rm, double* dSamples) {
    if (degree < 1 || degree > 12 || field.kind != kFieldMesh || maxTasks == 0 || maxTasks > 65535u) return hipErrorInvalidValue;
    const int nq = 4 * degree + 1;
    const unsigned gx = (unsigned)((nq * nq * nq + kMeshWg - 1) / kMeshWg);
    const uint32_t run = meshXcdRun();
    const unsigned gy = maxTasks + (8u * run + gx - 1u) / gx;  // whole groups of 8 runs of the XCD interleave past the last task
    if (gy > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(gx, gy), dim3(kMeshWg), 0, stream, dTasks, degree, dTables, field.mesh, rm, dSamples, dRange, 0u, run);
    return hipGetLastError();
}

HPSDF_FIT_KIND_UNIT(, kFieldMesh)

}  // namespace hpsdf
