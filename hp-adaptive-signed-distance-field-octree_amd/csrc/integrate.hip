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
//   integrate_reduce_kernel            256 rows -> 1 by the same tree, pass after pass until one row is left.
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

#include <rocprim/device/device_scan.hpp>

#include "dev_pool.hpp"
#include "device_types.hpp"
#include "integrate.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "runtime.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kIntThreads = kIntBlock;
constexpr int kRowStride = 16;  // doubles between two rows of a row array (15 used)

// v of lane t + N of the same row of 16 lanes (DPP row_shl:N); a lane whose source falls outside its row gets 0
template <int N>
__device__ __forceinline__ double rowShl(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x100 + N, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x100 + N, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// The header's tree over the workgroup's 256 rows, lane t holding row t: the sum ends in lane 0.  sRows: kIntRow x 128 doubles.
__device__ __forceinline__ void blockTree(double (&row)[kIntRow], double* sRows) {
    const uint32_t t = threadIdx.x;
    if (t >= 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) sRows[k * 128 + (t - 128u)] = row[k];
    __syncthreads();
    if (t < 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + sRows[k * 128 + t];
    __syncthreads();
    if (t >= 64u && t < 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) sRows[k * 128 + (t - 64u)] = row[k];
    __syncthreads();
    if (t < 64u) {
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + sRows[k * 128 + t];
        // lane t < stride reads lane t + stride < 2 stride, which held a valid sum after the step before; what the lanes above compute
        // is never read.  Strides 32 and 16 cross rows of 16 lanes (a lane permute); 8 .. 1 stay inside row 0: DPP row shifts
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + __shfl_down(row[k], 32, 64);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + __shfl_down(row[k], 16, 64);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<8>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<4>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<2>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<1>(row[k]);
    }
}

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

// rows in[0 .. n) -> out[0 .. ceil(n / 256)): workgroup b sums rows 256 b .. 256 b + 255, zero-padded
__global__ __launch_bounds__(kIntThreads) void integrate_reduce_kernel(const double* __restrict__ in, uint32_t n, double* __restrict__ out) {
    __shared__ double sRows[kIntRow * 128];
    const uint32_t i = blockIdx.x * kIntThreads + threadIdx.x;
    double row[kIntRow];
#pragma unroll
    for (int k = 0; k < kIntRow; ++k) row[k] = i < n ? in[(size_t)i * kRowStride + k] : 0.0;
    blockTree(row, sRows);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) out[(size_t)blockIdx.x * kRowStride + k] = row[k];
}

inline uint32_t blocksOf(uint32_t n) { return (n + kIntThreads - 1) / kIntThreads; }

// integrateLevels' lists on the device: the current list, and per level the flags, their ranks, the next list, the level's final cells and
// two row arrays; everything a level took but the next list is released when the level ends, everything when the call ends (DevPool)
struct DeviceIntegrateLists {
    hpsdf_ctx* ctx;
    const ClsTree& t;
    int maxDegree;
    const IntegrateArgs& a;
    DevPool pool{"hpsdf_integrate_device"};
    IntegrateCell* cur = nullptr;
    uint32_t* flags = nullptr;
    uint32_t* ranks = nullptr;
    uint32_t* notFinite = nullptr;

    int classify(int level, uint32_t n, uint32_t* nSplit, bool* finite) {
        hipStream_t s = ctx->stream;
        SURF_ALLOC(pool, flags, (size_t)n * 4, "split flags");
        SURF_ALLOC(pool, ranks, (size_t)n * 4, "split ranks");
        if (notFinite == nullptr) {
            SURF_ALLOC(pool, notFinite, 4, "flag");
            HPSDF_HIP(hipMemsetAsync(notFinite, 0, 4, s));
        }
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_classify_kernel<MAXP>), dim3(blocksOf(n)), dim3(kIntThreads), 0, s, t, ctx->dTables, cur, n, level, a.iso,
                               a.depth, flags, notFinite);
        });
        HPSDF_HIP(hipGetLastError());
        void* tmp = nullptr;
        size_t bytes = 0;
        const uint32_t* in = flags;
        uint32_t* out = ranks;
        if (const int rc = withTemp(pool, "rocprim::exclusive_scan", "scan storage", tmp, bytes, [=](void* p, size_t& b) {
                return rocprim::exclusive_scan(p, b, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
            }))
            return rc;
        uint32_t last[3] = {0, 0, 0};  // the last rank, the last flag, the flag of a non-finite cell
        HPSDF_HIP(hipMemcpyAsync(&last[0], ranks + (n - 1), 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(&last[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(&last[2], notFinite, 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(tmp);
        *nSplit = last[0] + last[1];
        *finite = last[2] == 0u;
        return HPSDF_OK;
    }

    int contribute(int level, uint32_t n, uint32_t nSplit, std::vector<IntegrateCell>* cells, double (&T)[kIntRow]) {
        hipStream_t s = ctx->stream;
        IntegrateCell* next = nullptr;
        IntegrateCell* finals = nullptr;
        double* rowsA = nullptr;
        double* rowsB = nullptr;
        const uint32_t nFinal = n - nSplit, nb = blocksOf(n);
        if (nSplit != 0) SURF_ALLOC(pool, next, (size_t)nSplit * 8 * sizeof(IntegrateCell), "the next list");
        if (cells != nullptr && nFinal != 0) SURF_ALLOC(pool, finals, (size_t)nFinal * sizeof(IntegrateCell), "final cells");
        SURF_ALLOC(pool, rowsA, (size_t)nb * kRowStride * sizeof(double), "rows");
        SURF_ALLOC(pool, rowsB, (size_t)blocksOf(nb) * kRowStride * sizeof(double), "rows");
        const uint32_t* r = nSplit != 0 ? ranks : nullptr;
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_contribute_kernel<MAXP>), dim3(nb), dim3(kIntThreads), 0, s, t, ctx->dTables, cur, n, level, a.iso, a.samples,
                               flags, r, next, finals, rowsA);
        });
        HPSDF_HIP(hipGetLastError());
        double* in = rowsA;
        double* out = rowsB;
        for (uint32_t m = nb; m > 1; m = blocksOf(m)) {  // (rowsB holds blocksOf(nb) rows, rowsA more: every pass fits)
            hipLaunchKernelGGL(integrate_reduce_kernel, dim3(blocksOf(m)), dim3(kIntThreads), 0, s, in, m, out);
            HPSDF_HIP(hipGetLastError());
            double* x = in;
            in = out, out = x;
        }
        HPSDF_HIP(hipMemcpyAsync(T, in, kIntRow * sizeof(double), hipMemcpyDeviceToHost, s));
        if (finals != nullptr) {
            const size_t at = cells->size();
            cells->resize(at + nFinal);
            HPSDF_HIP(hipMemcpyAsync(cells->data() + at, finals, (size_t)nFinal * sizeof(IntegrateCell), hipMemcpyDeviceToHost, s));
        }
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(finals), pool.release(rowsA), pool.release(rowsB), pool.release(flags), pool.release(ranks), pool.release(cur);
        cur = next;
        return HPSDF_OK;
    }
};

}  // namespace

// Integrate over a device tree: ct.consts are the tree's cached constants, dLeaves its cached list 0 (copied: a call writes classes into
// its lists).  Synchronises the context stream before it returns; frees everything it took, whatever happens.
int integrateOnDevice(hpsdf_ctx* ctx, const ClsTree& ct, int maxDegree, const IntegrateCell* dLeaves, uint32_t nLeaves, const IntegrateArgs& a,
                      hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    DeviceIntegrateLists L{ctx, ct, maxDegree, a};
    SURF_ALLOC(L.pool, L.cur, (size_t)nLeaves * sizeof(IntegrateCell), "list 0");
    HPSDF_HIP(hipMemcpyAsync(L.cur, dLeaves, (size_t)nLeaves * sizeof(IntegrateCell), hipMemcpyDeviceToDevice, ctx->stream));
    IntegrateSums S;
    const int rc = integrateLevels(L, a, nLeaves, outCells != nullptr, S);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call runs on when its arrays go)
        return rc;
    }
    hpsdf_integral r;
    integrateResult(S, ct.rootCentre, ct.rootInvSizes, a.samples, &r);
    return integrateHandOver(S, r, out, outCells, outCount);
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
