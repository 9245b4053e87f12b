// The part of the bit-exact fit that does not depend on the field kind: the workgroup shapes (fitLdsBytes, fitShape), pack_kernel, and
// the public launchFit / launchFitMulti / launchFieldEval, which check their arguments and switch on FieldDev::kind into
// fit_analytic.hip, fit_samples.hip or fit_mesh.hip (fit_kernels.hpp).  Nothing here takes long to compile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "device_types.hpp"
#include "fit_kernels.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"

namespace hpsdf {

// ---------------------------------------------------------------------------
// pack: Octree::ReallocCoeffs gather (Octree.cpp:510-552)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_kernel(const PackItem* __restrict__ items, uint32_t nItems,
                                                   const double* __restrict__ arena, double* __restrict__ out) {
    // one wave per leaf
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= nItems) return;
    const PackItem it = items[wave];
    for (uint32_t i = lane; i < it.count; i += 64) out[it.dst + i] = arena[it.src + i];
}

// ---------------------------------------------------------------------------
// launch wrappers (host)
// ---------------------------------------------------------------------------
size_t fitLdsBytes(int degree, int nTasks, int planes) {
    const size_t nq = 4 * (size_t)degree + 1;
    // sT + roots + weights + per-cell constants + `planes` sample planes per cell (also holds the new rows at the end)
    return ((size_t)(degree + 1) * nq + 2 * nq + 8 * (size_t)nTasks + (size_t)nTasks * planes * nq * nq) * sizeof(double);
}

// Shape of the workgroups of one class: `count` fits of `nrows` coefficient rows at `degree`.
FitShape fitShape(int degree, int nrows, uint32_t count, bool weighted, bool latencyBound) {
    FitShape sh;
    const int slots = nrows > kFitThreads ? 1 : kFitThreads / nrows;
    // Cell blocking (4 cells per thread sharing each basis product) is implemented in the kernel but measured
    // slower on MI355X (p=2, 65536 cells: 296 us vs 240 us): its 64 KB of LDS per workgroup leaves two workgroups
    // per CU to hide the phase barriers, and the kernel is not VALU-bound (52 % VALU-active).  Kept off.
    sh.cellsPerThread = 1;
    (void)count;
    int gmax = slots * sh.cellsPerThread;
    while (gmax > sh.cellsPerThread && fitLdsBytes(degree, gmax, 1) > kFitMaxLdsBytes) gmax -= sh.cellsPerThread;
    if (fitLdsBytes(degree, gmax, 1) > kFitMaxLdsBytes) {  // blocking does not fit: fall back
        sh.cellsPerThread = 1;
        gmax = slots;
        while (gmax > 1 && fitLdsBytes(degree, gmax, 1) > kFitMaxLdsBytes) --gmax;
    }
    // enough workgroups to cover the chip twice before cells are stacked into one workgroup
    int g = sh.cellsPerThread > 1 ? gmax
                                  : (int)std::min<uint32_t>((uint32_t)gmax, std::max<uint32_t>(1, (count + 511) / 512));
    // degree 2 (25 cells fit a workgroup): a round-0-sized launch is fastest at 4 cells per workgroup, big ones at 16
    // (tools/fit_shape_sweep.py: 4096 cells 53 -> 45 us; 32 768 cells 251 -> 211 us)
    if (degree == 2 && sh.cellsPerThread == 1)
        g = (int)std::min<uint32_t>(std::min(gmax, 16), std::max<uint32_t>(1, count <= 4096 ? (count + 1023) / 1024 : (count + 511) / 512));
    // Mesh fields: phase 1 is a chain of dependent BVH-node gathers per sample (measured on a 1.3 M-triangle mesh,
    // 4096 coarse cells: 206 ms with 8 cells per workgroup, 176 / 151 / 128 ms with 4 / 2 / 1) -- many small
    // workgroups keep more waves in flight and shorten the wait for the slowest lane of a chunk.
    if (latencyBound) g = 1;
    if (const char* e = std::getenv("HPSDF_FIT_G")) {  // tuning knobs
        sh.cellsPerThread = 1;
        g = std::max(1, std::min(slots, std::atoi(e)));
        while (g > 1 && fitLdsBytes(degree, g, 1) > kFitMaxLdsBytes) --g;
    }
    sh.cells = g;
    const int nq = 4 * degree + 1;
    const size_t budget = sh.cellsPerThread > 1 ? kFitMaxLdsBytes : kFitChunkLdsBytes;
    sh.planes = nq;
    while (sh.planes > 1 && fitLdsBytes(degree, g, sh.planes) > budget) --sh.planes;
    sh.ldsBytes = fitLdsBytes(degree, g, sh.planes);
    if (weighted) {
        // the sample region is reused for the full coefficient array + 100 FApprox values of every cell
        const int need = coeffCount(degree) + 100;
        const int minPlanes = (need + nq * nq - 1) / (nq * nq);
        sh.planes = std::max(sh.planes, std::min(nq, minPlanes));
        while (sh.cells > 1 && fitLdsBytes(degree, sh.cells, sh.planes) > kFitMaxLdsBytes) --sh.cells;
        sh.ldsBytes = fitLdsBytes(degree, sh.cells, sh.planes);
    }
    return sh;
}

// FN<kind>(...) of fit_kernels.hpp for a FieldDev
#define HPSDF_DISPATCH_KIND(FN, field, ...)                          \
    switch ((field).kind) {                                          \
        case kFieldAnalytic: FN<kFieldAnalytic>(__VA_ARGS__); break; \
        case kFieldSamples: FN<kFieldSamples>(__VA_ARGS__); break;   \
        default: FN<kFieldMesh>(__VA_ARGS__); break;                 \
    }

// every block of dBlocks[0 .. *dCount) -- or [0 .. maxBlocks) when dCount is null --, whatever its degree, in one launch;
// ldsBytes: the largest any of them needs
hipError_t launchFitMulti(hipStream_t stream, const FitBlock* dBlocks, uint32_t maxBlocks, size_t ldsBytes, const FitTask* dTasks,
                          double* dArena, double* dErrs, const DeviceTables* dTables, const FieldDev& field, const RootMap& rm,
                          const uint32_t* dCount) {
    if (maxBlocks == 0) return hipSuccess;
    if (ldsBytes > kFitMaxLdsBytes) return hipErrorInvalidValue;
    HPSDF_DISPATCH_KIND(launchFitMultiKind, field, stream, dBlocks, maxBlocks, ldsBytes, dTasks, dArena, dErrs, dTables, field, rm, dCount);
    return hipGetLastError();
}

hipError_t launchFit(hipStream_t stream, int degree, int cellsPerThread, const FitBlock* dBlocks, uint32_t nBlocks,
                     size_t ldsBytes, const FitTask* dTasks, double* dArena, double* dErrs, double* dMirror,
                     const DeviceTables* dTables, const FieldDev& field, const RootMap& rm, const uint32_t* dRange) {
    if (nBlocks == 0) return hipSuccess;
    if (ldsBytes > kFitMaxLdsBytes) return hipErrorInvalidValue;
    HPSDF_DISPATCH_KIND(launchFitKind, field, stream, degree, cellsPerThread, dBlocks, nBlocks, ldsBytes, dTasks, dArena,
                        dErrs, dMirror, dTables, field, rm, dRange);
    return hipGetLastError();
}

hipError_t launchFieldEval(hipStream_t stream, const FieldDev& f, const DeviceTables* dTables, const double* dXyz,
                           size_t n, double* dOut) {
    if (n == 0) return hipSuccess;
    HPSDF_DISPATCH_KIND(launchFieldKind, f, stream, f, dTables, dXyz, n, dOut);
    return hipGetLastError();
}

hipError_t launchPack(hipStream_t stream, const PackItem* dItems, uint32_t nItems, const double* dArena, double* dOut) {
    if (nItems == 0) return hipSuccess;
    const unsigned blocks = (nItems + 3) / 4;  // 4 waves per block
    hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, stream, dItems, nItems, dArena, dOut);
    return hipGetLastError();
}

}  // namespace hpsdf
