// Clearance: a branch-and-bound search over tree A's cells for the minimum of tree B's field over A's solid under an affine pose
// (include/hpsdf.h, "Clearance"; the cell's statements, the prune test and the level loop are clearance.hpp's).  A level is
//
//   clearance_bound_kernel<MAXP>   one lane per cell of the current list: A's class, the cell's image box and QueryBounds' walk of B over
//                                  it (its stack in LDS, [level][lane] as in integrate_pair.hip), Query of A at the cell's centre and of B
//                                  at its image.  The cell's blo goes to memory; the (vb, pos) minimum of the workgroup's 256 lanes is
//                                  reduced in LDS, then by shuffles and DPP row shifts, into one row a workgroup.
//   clearance_fold_kernel          256 rows -> one, pass after pass; the last pass (one workgroup) replaces the running best in device
//                                  memory iff the level's candidate is strictly below it, and keeps the candidate's cell.
//   clearance_prune_kernel         one lane per cell: the cell's kind from blo and the best just written (no host round trip), the scan's
//                                  input word (a split candidate 1, a final 2^32) and a row a workgroup: the least blo of the finals and of
//                                  the split candidates, and the four counts.
//   clearance_sum_kernel           those rows -> one, the last pass into the call's state.
//   rocprim::exclusive_scan        over the 64-bit words: both ranks of a cell in one scan.
//   one read-back                  the state: best and its cell, L's two parts, the counts, the not-finite word.
//   clearance_emit_kernel          the split candidates' children into the next list, the finals and their blo into the level's arrays.
//
// No atomic decides a value: every minimum is a lexicographic or plain minimum, which does not depend on the order, and the counts are
// integers in doubles.  One DevEval<MAXP> serves both trees, as in integrate_pair.hip.  Built with -ffp-contract=off like every other
// unit: hostClearance (clearance_host.cpp) gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "clearance.hpp"
#include "clearance_dev.hpp"
#include "dev_pool.hpp"
#include "device_types.hpp"
#include "integrate.hpp"
#include "integrate_pair.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "runtime.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

constexpr int kClrSums = 6;  // minFinal, minSplit, outside, pruned, split, final

// the call's state in device memory: written by the last pass of the two reductions, read back once a level
struct ClearanceState {
    double best, bestVa;
    IntegrateCell bestCell;
    uint32_t hasWitness;
    double sums[kClrSums];
    uint32_t notFinite, pad;
};

// v of lane t + N of the same row of 16 lanes (DPP row_shl:N); a lane whose source falls outside its row gets 0
template <int N>
__device__ __forceinline__ uint32_t rowShlU(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xF, 0xF, false);
}
template <int N>
__device__ __forceinline__ double rowShlD(double v) {
    return __hiloint2double((int)rowShlU<N>((uint32_t)__double2hiint(v)), (int)rowShlU<N>((uint32_t)__double2loint(v)));
}

__device__ __forceinline__ void candTake(ClearanceCandidate& c, double vb, double va, uint32_t pos) {
    if (clearanceBefore(vb, pos, c.vb, c.pos)) c.vb = vb, c.va = va, c.pos = pos;
}

// The lexicographic minimum of (vb, pos) over the workgroup's 256 lanes, ending in lane 0: integrate_dev.hpp's tree -- LDS for the
// strides 128 and 64, lane permutes for 32 and 16, DPP row shifts inside row 0 for 8 .. 1 (a lane t < stride reads lane t + stride, which
// held a valid candidate after the step before; what the lanes above compute is never read).  sV, sA: 128 doubles, sP: 128 words.
__device__ __forceinline__ void blockCandidate(ClearanceCandidate& c, double* sV, double* sA, uint32_t* sP) {
    const uint32_t t = threadIdx.x;
    if (t >= 128u) sV[t - 128u] = c.vb, sA[t - 128u] = c.va, sP[t - 128u] = c.pos;
    __syncthreads();
    if (t < 128u) candTake(c, sV[t], sA[t], sP[t]);
    __syncthreads();
    if (t >= 64u && t < 128u) sV[t - 64u] = c.vb, sA[t - 64u] = c.va, sP[t - 64u] = c.pos;
    __syncthreads();
    if (t < 64u) {
        candTake(c, sV[t], sA[t], sP[t]);
        {
            const double vb = __shfl_down(c.vb, 32, 64), va = __shfl_down(c.va, 32, 64);
            const uint32_t pos = __shfl_down(c.pos, 32, 64);
            candTake(c, vb, va, pos);
        }
        {
            const double vb = __shfl_down(c.vb, 16, 64), va = __shfl_down(c.va, 16, 64);
            const uint32_t pos = __shfl_down(c.pos, 16, 64);
            candTake(c, vb, va, pos);
        }
#define HPSDF_CLR_STEP(N)                                                                    \
    {                                                                                        \
        const double vb = rowShlD<N>(c.vb), va = rowShlD<N>(c.va);                           \
        const uint32_t pos = rowShlU<N>(c.pos);                                              \
        candTake(c, vb, va, pos);                                                            \
    }
        HPSDF_CLR_STEP(8)
        HPSDF_CLR_STEP(4)
        HPSDF_CLR_STEP(2)
        HPSDF_CLR_STEP(1)
#undef HPSDF_CLR_STEP
    }
}

template <int MAXP>
__global__ __launch_bounds__(kClrThreads) void clearance_bound_kernel(ClsTree tA, ClsTree tB, PairArgs a, const DeviceTables* __restrict__ T,
                                                                      IntegrateCell* __restrict__ list, uint32_t n, int level,
                                                                      double* __restrict__ blo, ClearanceCandidate* __restrict__ rows,
                                                                      ClearanceState* __restrict__ state) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint32_t sFirst[kLevels * kClrThreads];
    __shared__ uint8_t sMask[kLevels * kClrThreads];
    __shared__ double sV[128];
    __shared__ double sA[128];
    __shared__ uint32_t sP[128];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    LdsClrStack st{sFirst + threadIdx.x, sMask + threadIdx.x};
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    ClearanceCandidate cand{boundsInf(), 0.0, kClearanceNoPos};
    if (i < n) {
        const IntegrateCell c = list[i];
        bool finite = true;
        ClearanceCell o;
        clearanceCell(tA, tB, a, c, level, eval, st, &finite, o);
        list[i].cls = (uint8_t)o.clsA;
        blo[i] = o.blo;
        cand.vb = o.vb, cand.va = o.va, cand.pos = i;
        if (!finite) state->notFinite = 1u;  // (every writer stores the same word)
    }
    blockCandidate(cand, sV, sA, sP);
    if (threadIdx.x == 0) rows[blockIdx.x] = cand;
}

// rows in[0 .. n) -> out[0 .. ceil(n / 256)); last (one workgroup): the level's candidate against the running best (step 2's last line)
__global__ __launch_bounds__(kClrThreads) void clearance_fold_kernel(const ClearanceCandidate* __restrict__ in, uint32_t n,
                                                                     ClearanceCandidate* __restrict__ out, int last,
                                                                     const IntegrateCell* __restrict__ list, ClearanceState* __restrict__ state) {
    __shared__ double sV[128];
    __shared__ double sA[128];
    __shared__ uint32_t sP[128];
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    ClearanceCandidate cand{boundsInf(), 0.0, kClearanceNoPos};
    if (i < n) cand = in[i];
    blockCandidate(cand, sV, sA, sP);
    if (threadIdx.x != 0) return;
    if (!last) {
        out[blockIdx.x] = cand;
        return;
    }
    if (cand.vb < state->best) {  // (a candidate has a position: vb < +inf)
        state->best = cand.vb, state->bestVa = cand.va;
        state->bestCell = list[cand.pos];
        state->hasWitness = 1u;
    }
}

// the six sums of a workgroup's lanes, ending in lane 0: two minima and four counts, by the same tree.  s: kClrSums x 128 doubles
__device__ __forceinline__ void sumTake(double (&x)[kClrSums], const double (&y)[kClrSums]) {
    x[0] = y[0] < x[0] ? y[0] : x[0];
    x[1] = y[1] < x[1] ? y[1] : x[1];
#pragma unroll
    for (int k = 2; k < kClrSums; ++k) x[k] = x[k] + y[k];
}
__device__ __forceinline__ void blockSums(double (&x)[kClrSums], double* s) {
    const uint32_t t = threadIdx.x;
    double y[kClrSums];
    if (t >= 128u)
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) s[k * 128 + (t - 128u)] = x[k];
    __syncthreads();
    if (t < 128u) {
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = s[k * 128 + t];
        sumTake(x, y);
    }
    __syncthreads();
    if (t >= 64u && t < 128u)
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) s[k * 128 + (t - 64u)] = x[k];
    __syncthreads();
    if (t < 64u) {
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = s[k * 128 + t];
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = __shfl_down(x[k], 32, 64);
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = __shfl_down(x[k], 16, 64);
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = rowShlD<8>(x[k]);
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = rowShlD<4>(x[k]);
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = rowShlD<2>(x[k]);
        sumTake(x, y);
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) y[k] = rowShlD<1>(x[k]);
        sumTake(x, y);
    }
}

__device__ __forceinline__ void sumsNone(double (&x)[kClrSums]) {
    x[0] = x[1] = boundsInf();
#pragma unroll
    for (int k = 2; k < kClrSums; ++k) x[k] = 0.0;
}

// Step 3 of every cell with the best the fold left in the state; rows: kClrSums doubles a workgroup
__global__ __launch_bounds__(kClrThreads) void clearance_prune_kernel(const IntegrateCell* __restrict__ list, const double* __restrict__ blo, uint32_t n,
                                                                      uint32_t maxDepth, const ClearanceState* __restrict__ state,
                                                                      unsigned long long* __restrict__ flags, double* __restrict__ rows) {
    __shared__ double s[kClrSums * 128];
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    double x[kClrSums];
    sumsNone(x);
    if (i < n) {
        const IntegrateCell c = list[i];
        const double b = blo[i];
        const uint32_t kind = clearanceKind(c.cls, b, state->best, c.depth, maxDepth);
        flags[i] = kind == kClearSplit ? 1ull : (kind == kClearFinal ? 1ull << 32 : 0ull);
        if (kind == kClearFinal) x[0] = b;
        if (kind == kClearSplit) x[1] = b;
        x[2 + kind] = 1.0;
    }
    blockSums(x, s);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) rows[(size_t)blockIdx.x * kClrSums + k] = x[k];
}

// the slot of a kind in a row of sums: kClearOutside .. kClearFinal are 0 .. 3 and follow the two minima
static_assert(kClearOutside == 0u && kClearPruned == 1u && kClearSplit == 2u && kClearFinal == 3u, "clearance_prune_kernel counts by kind");

__global__ __launch_bounds__(kClrThreads) void clearance_sum_kernel(const double* __restrict__ in, uint32_t n, double* __restrict__ out, int last,
                                                                    ClearanceState* __restrict__ state) {
    __shared__ double s[kClrSums * 128];
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    double x[kClrSums];
    sumsNone(x);
    if (i < n)
#pragma unroll
        for (int k = 0; k < kClrSums; ++k) x[k] = in[(size_t)i * kClrSums + k];
    blockSums(x, s);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < kClrSums; ++k) {
        if (last) state->sums[k] = x[k];
        else out[(size_t)blockIdx.x * kClrSums + k] = x[k];
    }
}

// ranks: the exclusive scan of flags (low word: split candidates before the cell, high word: finals).  split: next holds 8 cells per
// split candidate and the finals are the cells at the depth limit; else every survivor is final.
__global__ __launch_bounds__(kClrThreads) void clearance_emit_kernel(const IntegrateCell* __restrict__ list, const double* __restrict__ blo, uint32_t n,
                                                                     const unsigned long long* __restrict__ flags,
                                                                     const unsigned long long* __restrict__ ranks, int split,
                                                                     IntegrateCell* __restrict__ next, IntegrateCell* __restrict__ finals,
                                                                     double* __restrict__ finalBlo) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long f = flags[i];
    if (f == 0ull) return;
    const unsigned long long r = ranks[i];
    const uint32_t rs = (uint32_t)r, rf = (uint32_t)(r >> 32);
    const IntegrateCell c = list[i];
    if (split && f == 1ull) {
        for (uint32_t ch = 0; ch < 8u; ++ch) next[8u * rs + ch] = integrateChild(c, ch);
        return;
    }
    const uint32_t at = split ? rf : rs + rf;
    if (finals != nullptr) finals[at] = c;
    finalBlo[at] = blo[i];
}

// clearanceLevels' lists on the device
struct DeviceClearanceLists {
    hpsdf_ctx* ctx;
    const ClsTree& tA;
    const ClsTree& tB;
    const PairArgs& p;
    int maxDegree;
    uint32_t maxDepth;
    DevPool pool;
    IntegrateCell* cur = nullptr;
    double* blo = nullptr;
    unsigned long long* flags = nullptr;
    unsigned long long* ranks = nullptr;
    ClearanceState* state = nullptr;
    ClearanceState host{};  // the state's first value and every level's read-back

    int start(const IntegrateCell* dLeaves, uint32_t nLeaves) {
        hipStream_t s = ctx->stream;
        SURF_ALLOC(pool, cur, (size_t)nLeaves * sizeof(IntegrateCell), "list 0");
        SURF_ALLOC(pool, state, sizeof(ClearanceState), "state");
        HPSDF_HIP(hipMemcpyAsync(cur, dLeaves, (size_t)nLeaves * sizeof(IntegrateCell), hipMemcpyDeviceToDevice, s));
        host = ClearanceState{};
        host.best = boundsInf();
        HPSDF_HIP(hipMemcpyAsync(state, &host, sizeof host, hipMemcpyHostToDevice, s));
        HPSDF_HIP(hipStreamSynchronize(s));  // (host is written again by the first read-back)
        return HPSDF_OK;
    }

    int level(int level, uint32_t n, ClearanceLevel* v) {
        hipStream_t s = ctx->stream;
        const uint32_t nb = clrBlocks(n);
        ClearanceCandidate* candA = nullptr;
        ClearanceCandidate* candB = nullptr;
        double* sumA = nullptr;
        double* sumB = nullptr;
        SURF_ALLOC(pool, blo, (size_t)n * sizeof(double), "cell bounds");
        SURF_ALLOC(pool, flags, (size_t)n * 8, "flags");
        SURF_ALLOC(pool, ranks, (size_t)n * 8, "ranks");
        SURF_ALLOC(pool, candA, (size_t)nb * sizeof(ClearanceCandidate), "candidate rows");
        SURF_ALLOC(pool, candB, (size_t)clrBlocks(nb) * sizeof(ClearanceCandidate), "candidate rows");
        SURF_ALLOC(pool, sumA, (size_t)nb * kClrSums * sizeof(double), "rows");
        SURF_ALLOC(pool, sumB, (size_t)clrBlocks(nb) * kClrSums * sizeof(double), "rows");
        forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
            constexpr int MAXP = decltype(P)::value;
            hipLaunchKernelGGL((clearance_bound_kernel<MAXP>), dim3(nb), dim3(kClrThreads), 0, s, tA, tB, p, ctx->dTables, cur, n, level, blo, candA,
                               state);
        });
        HPSDF_HIP(hipGetLastError());
        {
            ClearanceCandidate* in = candA;
            ClearanceCandidate* out = candB;
            for (uint32_t m = nb;; m = clrBlocks(m)) {  // (candB holds clrBlocks(nb) rows, candA more: every pass fits)
                const int last = clrBlocks(m) == 1u;
                hipLaunchKernelGGL(clearance_fold_kernel, dim3(clrBlocks(m)), dim3(kClrThreads), 0, s, in, m, out, last, cur, state);
                HPSDF_HIP(hipGetLastError());
                if (last) break;
                ClearanceCandidate* x = in;
                in = out, out = x;
            }
        }
        hipLaunchKernelGGL(clearance_prune_kernel, dim3(nb), dim3(kClrThreads), 0, s, cur, blo, n, maxDepth, state, flags, sumA);
        HPSDF_HIP(hipGetLastError());
        {
            double* in = sumA;
            double* out = sumB;
            for (uint32_t m = nb;; m = clrBlocks(m)) {
                const int last = clrBlocks(m) == 1u;
                hipLaunchKernelGGL(clearance_sum_kernel, dim3(clrBlocks(m)), dim3(kClrThreads), 0, s, in, m, out, last, state);
                HPSDF_HIP(hipGetLastError());
                if (last) break;
                double* x = in;
                in = out, out = x;
            }
        }
        void* tmp = nullptr;
        size_t bytes = 0;
        const unsigned long long* in = flags;
        unsigned long long* out = ranks;
        if (const int rc = withTemp(pool, "rocprim::exclusive_scan", "scan storage", tmp, bytes, [=](void* q, size_t& b) {
                return rocprim::exclusive_scan(q, b, in, out, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), s);
            }))
            return rc;
        HPSDF_HIP(hipMemcpyAsync(&host, state, sizeof host, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(tmp), pool.release(candA), pool.release(candB), pool.release(sumA), pool.release(sumB);
        v->best = host.best, v->bestVa = host.bestVa, v->bestCell = host.bestCell, v->hasWitness = host.hasWitness;
        v->minFinal = host.sums[0], v->minSplit = host.sums[1];
        v->nOutside = (uint64_t)host.sums[2], v->nPruned = (uint64_t)host.sums[3];
        v->nSplit = (uint64_t)host.sums[4], v->nFinal = (uint64_t)host.sums[5];
        v->finite = host.notFinite == 0u;
        return HPSDF_OK;
    }

    int emit(int, uint32_t n, bool split, uint32_t nSplit, uint32_t nFinal, std::vector<IntegrateCell>* cells, std::vector<double>& finalBlo) {
        hipStream_t s = ctx->stream;
        IntegrateCell* next = nullptr;
        IntegrateCell* finals = nullptr;
        double* fb = nullptr;
        const uint32_t nf = split ? nFinal : nSplit + nFinal;
        if (split) SURF_ALLOC(pool, next, (size_t)nSplit * 8 * sizeof(IntegrateCell), "the next list");
        if (cells != nullptr && nf != 0) SURF_ALLOC(pool, finals, (size_t)nf * sizeof(IntegrateCell), "final cells");
        if (nf != 0) SURF_ALLOC(pool, fb, (size_t)nf * sizeof(double), "final bounds");
        if (split || nf != 0) {
            hipLaunchKernelGGL(clearance_emit_kernel, dim3(clrBlocks(n)), dim3(kClrThreads), 0, s, cur, blo, n, flags, ranks, split ? 1 : 0, next,
                               finals, fb);
            HPSDF_HIP(hipGetLastError());
        }
        if (nf != 0) {
            const size_t at = finalBlo.size();
            finalBlo.resize(at + nf);
            HPSDF_HIP(hipMemcpyAsync(finalBlo.data() + at, fb, (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, s));
            if (finals != nullptr) {
                cells->resize(at + nf);  // (cells and finalBlo grow together)
                HPSDF_HIP(hipMemcpyAsync(cells->data() + at, finals, (size_t)nf * sizeof(IntegrateCell), hipMemcpyDeviceToHost, s));
            }
        }
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(finals), pool.release(fb), pool.release(blo), pool.release(flags), pool.release(ranks), pool.release(cur);
        cur = next;
        return HPSDF_OK;
    }
};

}  // namespace

// Clearance over two device trees of one device: ctA.consts and ctB.consts are the trees' cached constants, dLeaves is A's cached list 0.
// Synchronises the context stream before it returns; frees everything it took, whatever happens.
int clearanceOnDevice(hpsdf_ctx* ctx, const ClsTree& ctA, const ClsTree& ctB, int maxDegree, const IntegrateCell* dLeaves, uint32_t nLeaves,
                      const PairArgs& p, const ClearanceArgs& a, hpsdf_clearance* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    DeviceClearanceLists L{ctx, ctA, ctB, p, maxDegree, a.depth, DevPool{"hpsdf_clearance_device"}};
    ClearanceSums S;
    int rc = nLeaves != 0 ? L.start(dLeaves, nLeaves) : HPSDF_OK;
    // the witness's point and image are made on the host from its cell by the kernels' statements: no tree is read for them
    if (!rc) rc = clearanceLevels(L, ctA, p, a, nLeaves, outCells != nullptr, S);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call runs on when its arrays go)
        return rc;
    }
    return clearanceHandOver(S, out, outCells, outCount);
}

}  // namespace hpsdf
