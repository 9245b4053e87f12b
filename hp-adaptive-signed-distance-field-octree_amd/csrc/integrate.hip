// Integrate: volume bounds and moments of {Query < iso} over the root by level-by-level refinement of the leaves into dyadic cells
// (include/hpsdf.h, "Integrate"; the cell's statements and the level loop are integrate.hpp's, the leaf evaluation is Query's evalLeaf).
//
//   integrate_classify_kernel<MAXP>    one lane per cell of the current list: one evaluation at the cell's centre, the class byte into the
//                                      cell's record, the split flag (undecided and above the depth limit) as a 32-bit word for the scan.
//   (rocprim::exclusive_scan)          the split flags -> each split cell's rank: its children go to 8 rank .. 8 rank + 7 of the next list,
//                                      a final cell to i - rank of the level's final cells.  No atomic decides a position.
//   integrate_contribute_kernel<MAXP>  one lane per cell, one workgroup per 256 cells in list order: a split cell writes its 8 children,
//                                      a final cell makes its row (box moments, or the q^3 samples of an undecided cell) in registers;
//                                      the workgroup's 256 rows are summed by the header's tree -- strides 128 and 64 through LDS (the
//                                      upper half of the lanes stores, the lower half adds), strides 32 and 16 inside wave 0 by lane
//                                      permutes, 8 .. 1 by DPP row shifts -- and ONE row per workgroup is written.  No per-cell row array exists.
//   integrate_reduce_kernel            256 rows -> 1 by the same tree, pass after pass until one row is left (integrate_dev.hpp, with the
//                                      tree itself and the lists' driver: IntegratePair uses the same ones).
//
// Memory per cell of a level: 12 bytes (its record) + 4 (flag) + 4 (rank), 12 more per child made and, when the caller asks for the
// cells, 12 per final cell until the level's cells are downloaded; 120 bytes per 256 cells of rows.  max_cells bounds every list but
// list 0 (the leaves).  A wave's lanes mostly share a leaf (the 8 children of a cell are neighbours in the list, and so are theirs), so
// their coefficient loads fall on the same 128-byte lines: a wave of 64 cells of one degree-2 leaf fetches one line, not 64.
//
// List 0 (the leaves with their depth and integer coordinates) depends on the tree alone: hpsdf_tree::integrateLeaves makes it at the
// first call, under the lock that guards the leaves' constants, and the tree keeps it.
//
// Built with -ffp-contract=off like every other unit: hostIntegrate (host_query.cpp) gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "device_types.hpp"
#include "integrate.hpp"
#include "integrate_dev.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "runtime.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

template <int MAXP>
__global__ __launch_bounds__(kIntThreads) void integrate_classify_kernel(ClsTree t, const DeviceTables* __restrict__ T, IntegrateCell* __restrict__ list,
                                                                         uint32_t n, int level, double iso, uint32_t maxDepth,
                                                                         uint32_t* __restrict__ flags, uint32_t* __restrict__ notFinite) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    const uint32_t i = blockIdx.x * kIntThreads + threadIdx.x;
    if (i >= n) return;
    const IntegrateCell c = list[i];
    bool finite = true;
    const uint32_t cls = integrateCellClass(t, c, level, iso, eval, &finite);
    list[i].cls = (uint8_t)cls;
    flags[i] = cls == 0u && c.depth < maxDepth ? 1u : 0u;
    if (!finite) *notFinite = 1u;  // (every writer stores the same word)
}

// ranks == nullptr: no cell of this level is split.  next holds 8 cells per split cell, finals (may be null) one per final cell, rows one
// row per workgroup.
template <int MAXP>
__global__ __launch_bounds__(kIntThreads) void integrate_contribute_kernel(ClsTree t, const DeviceTables* __restrict__ T, const IntegrateCell* __restrict__ list,
                                                                           uint32_t n, int level, double iso, uint32_t q,
                                                                           const uint32_t* __restrict__ flags, const uint32_t* __restrict__ ranks,
                                                                           IntegrateCell* __restrict__ next, IntegrateCell* __restrict__ finals,
                                                                           double* __restrict__ rows) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ double sRows[kIntRow * 128];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    const uint32_t i = blockIdx.x * kIntThreads + threadIdx.x;
    double row[kIntRow];
#pragma unroll
    for (int k = 0; k < kIntRow; ++k) row[k] = 0.0;
    if (i < n) {
        const IntegrateCell c = list[i];
        const uint32_t rank = ranks != nullptr ? ranks[i] : 0u;
        if (ranks != nullptr && flags[i] != 0u) {
            for (uint32_t ch = 0; ch < 8u; ++ch) next[8u * rank + ch] = integrateChild(c, ch);
        } else {
            integrateCellRow(t, c, level, iso, q, eval, row);
            if (finals != nullptr) finals[i - rank] = c;
        }
    }
    blockTree(row, sRows);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) rows[(size_t)blockIdx.x * kRowStride + k] = row[k];
}

// a level's two launches (integrate_dev.hpp, DeviceIntegrateLists)
struct IntegrateKernels {
    const ClsTree& t;
    const DeviceTables* dTables;
    int maxDegree;
    const IntegrateArgs& a;

    void classify(hipStream_t s, IntegrateCell* cur, uint32_t n, int level, uint32_t* flags, uint32_t* notFinite) const {
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_classify_kernel<MAXP>), dim3(blocksOf(n)), dim3(kIntThreads), 0, s, t, dTables, cur, n, level, a.iso, a.depth,
                               flags, notFinite);
        });
    }
    void contribute(hipStream_t s, const IntegrateCell* cur, uint32_t n, int level, const uint32_t* flags, const uint32_t* ranks, IntegrateCell* next,
                    IntegrateCell* finals, double* rows) const {
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_contribute_kernel<MAXP>), dim3(blocksOf(n)), dim3(kIntThreads), 0, s, t, dTables, cur, n, level, a.iso,
                               a.samples, flags, ranks, next, finals, rows);
        });
    }
};

}  // namespace

// Integrate over a device tree: ct.consts are the tree's cached constants, dLeaves its cached list 0 (copied: a call writes classes into
// its lists).  Synchronises the context stream before it returns; frees everything it took, whatever happens.
int integrateOnDevice(hpsdf_ctx* ctx, const ClsTree& ct, int maxDegree, const IntegrateCell* dLeaves, uint32_t nLeaves, const IntegrateArgs& a,
                      hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    const IntegrateKernels kernels{ct, ctx->dTables, maxDegree, a};
    DeviceIntegrateLists<IntegrateKernels> L{ctx, kernels, DevPool{"hpsdf_integrate_device"}};
    return L.run(dLeaves, nLeaves, a, ct.rootCentre, ct.rootInvSizes, out, outCells, outCount);
}

}  // namespace hpsdf

using namespace hpsdf;

// List 0 of this tree on its device, made once: from the host copy of the records (hostCopies), by integrateLeafCells, under boundLock.
int hpsdf_tree::integrateLeaves(hpsdf_ctx* ctx) const {
    if (leafCellsReady.load(std::memory_order_acquire)) return HPSDF_OK;
    if (const int rc = hostCopies()) return rc;
    std::lock_guard<std::mutex> guard(boundLock);
    if (leafCellsReady.load(std::memory_order_relaxed)) return HPSDF_OK;
    HPSDF_HIP(hipSetDevice(device));
    std::vector<IntegrateCell> cells;
    integrateLeafCells(hRecs.data(), hRecs.size(), cells);
    if (cells.empty()) return fail(HPSDF_ERR_STATE, "hpsdf_integrate: a tree without leaves");
    IntegrateCell* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, cells.size() * sizeof(IntegrateCell));
    if (e == hipSuccess) e = hipMemcpy(d, cells.data(), cells.size() * sizeof(IntegrateCell), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_integrate: out of device memory (list 0)");
        }
        return hipFail(e, "list 0");
    }
    (void)ctx;
    dLeafCells = d;
    nLeafCells = (uint32_t)cells.size();
    leafCellsReady.store(true, std::memory_order_release);
    return HPSDF_OK;
}
