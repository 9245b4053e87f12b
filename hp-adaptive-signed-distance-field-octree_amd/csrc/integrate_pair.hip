// IntegratePair: Integrate's level-by-level refinement of tree A's leaves, with every cell also classified against tree B under an affine
// pose (include/hpsdf.h, "IntegratePair"; the cell's statements are integrate_pair.hpp's, the lists, the scan and the row reduction are
// Integrate's, integrate_dev.hpp).
//
//   integrate_pair_classify_kernel<MAXP>    one lane per cell of the current list: A's class at one evaluation of A's leaf; where that does
//                                           not decide the operation, the cell's image box in B's frame and QueryBounds' walk of B over it
//                                           (boundsWalkRange, subdiv 1).  The walk's stack is in LDS, indexed [level][lane] as in
//                                           query_bounds.hip: kLevels x 256 x 5 bytes a workgroup, no scratch.  A lane walks until its box
//                                           is done: a wave costs its slowest lane (no compaction, no wave cooperating on one walk).
//   integrate_pair_contribute_kernel<MAXP>  integrate_contribute_kernel with pairCellRow: an undecided final cell evaluates A at its q^3
//                                           sub-box centres and, where A alone does not decide the predicate, descends B to the image point.
// One DevEval<MAXP> serves both trees: MAXP is the class of the larger of the two trees' maximum degrees (three instantiations a kernel).
// Both trees' constants and A's list 0 are the trees' own caches (hpsdf_tree::boundConsts, integrateLeaves).
//
// Built with -ffp-contract=off like every other unit: hostIntegratePair (integrate_pair_host.cpp) gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "integrate.hpp"
#include "integrate_dev.hpp"
#include "integrate_pair.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "runtime.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

// boundsWalkRange's Stack in LDS: level d of this lane at [d * kIntThreads + lane]
struct LdsPairStack {
    uint32_t* f;
    uint8_t* m;
    __device__ __forceinline__ uint32_t first(int d) const { return f[d * kIntThreads]; }
    __device__ __forceinline__ uint32_t mask(int d) const { return m[d * kIntThreads]; }
    __device__ __forceinline__ void setFirst(int d, uint32_t v) { f[d * kIntThreads] = v; }
    __device__ __forceinline__ void setMask(int d, uint32_t v) { m[d * kIntThreads] = (uint8_t)v; }
};

template <int MAXP>
__global__ __launch_bounds__(kIntThreads) void integrate_pair_classify_kernel(ClsTree tA, ClsTree tB, PairArgs a, const DeviceTables* __restrict__ T,
                                                                              IntegrateCell* __restrict__ list, uint32_t n, int level,
                                                                              uint32_t maxDepth, uint32_t* __restrict__ flags,
                                                                              uint32_t* __restrict__ notFinite) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint32_t sFirst[kLevels * kIntThreads];
    __shared__ uint8_t sMask[kLevels * kIntThreads];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    LdsPairStack st{sFirst + threadIdx.x, sMask + threadIdx.x};
    const uint32_t i = blockIdx.x * kIntThreads + threadIdx.x;
    if (i >= n) return;
    const IntegrateCell c = list[i];
    bool finite = true;
    const uint32_t cls = pairCellClass(tA, tB, a, c, level, eval, st, &finite);
    list[i].cls = (uint8_t)cls;
    flags[i] = cls == 0u && c.depth < maxDepth ? 1u : 0u;
    if (!finite) *notFinite = 1u;  // (every writer stores the same word)
}

// ranks == nullptr: no cell of this level is split.  next holds 8 cells per split cell, finals (may be null) one per final cell, rows one
// row per workgroup.
template <int MAXP>
__global__ __launch_bounds__(kIntThreads) void integrate_pair_contribute_kernel(ClsTree tA, ClsTree tB, PairArgs a, const DeviceTables* __restrict__ T,
                                                                                const IntegrateCell* __restrict__ list, uint32_t n, int level,
                                                                                uint32_t q, const uint32_t* __restrict__ flags,
                                                                                const uint32_t* __restrict__ ranks, IntegrateCell* __restrict__ next,
                                                                                IntegrateCell* __restrict__ finals, double* __restrict__ rows) {
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
            pairCellRow(tA, tB, a, c, level, q, eval, row);
            if (finals != nullptr) finals[i - rank] = c;
        }
    }
    blockTree(row, sRows);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) rows[(size_t)blockIdx.x * kRowStride + k] = row[k];
}

// a level's two launches (integrate_dev.hpp, DeviceIntegrateLists)
struct PairKernels {
    const ClsTree& tA;
    const ClsTree& tB;
    const PairArgs& p;
    const DeviceTables* dTables;
    int maxDegree;  // of both trees
    const IntegrateArgs& a;

    void classify(hipStream_t s, IntegrateCell* cur, uint32_t n, int level, uint32_t* flags, uint32_t* notFinite) const {
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_pair_classify_kernel<MAXP>), dim3(blocksOf(n)), dim3(kIntThreads), 0, s, tA, tB, p, dTables, cur, n, level,
                               a.depth, flags, notFinite);
        });
    }
    void contribute(hipStream_t s, const IntegrateCell* cur, uint32_t n, int level, const uint32_t* flags, const uint32_t* ranks, IntegrateCell* next,
                    IntegrateCell* finals, double* rows) const {
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((integrate_pair_contribute_kernel<MAXP>), dim3(blocksOf(n)), dim3(kIntThreads), 0, s, tA, tB, p, dTables, cur, n, level,
                               a.samples, flags, ranks, next, finals, rows);
        });
    }
};

}  // namespace

// IntegratePair over two device trees of one device: ctA.consts and ctB.consts are the trees' cached constants, dLeaves is A's cached list 0.
// Synchronises the context stream before it returns; frees everything it took, whatever happens.
int integratePairOnDevice(hpsdf_ctx* ctx, const ClsTree& ctA, const ClsTree& ctB, int maxDegree, const IntegrateCell* dLeaves, uint32_t nLeaves,
                          const PairArgs& p, const IntegrateArgs& a, hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    const PairKernels kernels{ctA, ctB, p, ctx->dTables, maxDegree, a};
    DeviceIntegrateLists<PairKernels> L{ctx, kernels, DevPool{"hpsdf_integrate_pair_device"}};
    return L.run(dLeaves, nLeaves, a, ctA.rootCentre, ctA.rootInvSizes, out, outCells, outCount);
}

}  // namespace hpsdf
