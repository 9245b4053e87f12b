// ClearanceBatch: Clearance (clearance.hip; include/hpsdf.h, "Clearance", "Batches") for many poses of the same two trees at once.  The
// lists of a chunk's poses are ONE list: a pose's cells are a contiguous run, the runs in pose order, each in the single call's order,
// with a parallel pose index.  The levels run in lockstep (clearanceCell's `level` is global); a pose that has stopped has no cells.
// Every pose has a row of state in device memory (ClearanceBatchPose) and its PairArgs there.  A level is
//
//   clearance_batch_bound_kernel<MAXP>  one lane per cell: clearance_bound_kernel's statements with the pose's arguments read from
//                                       memory; blo, vb and va go to memory; the least key of vb into the pose's row.
//   clearance_batch_pick_kernel         one lane per cell: among the holders of the pose's least key, the least position IN THE POSE'S
//                                       OWN RUN -- the lexicographic minimum of (vb, pos), clearanceBefore's.
//   clearance_batch_prune_kernel        one lane per cell: its kind against the pose's updated best (the old best and the candidate just
//                                       picked: step 2's last line, read-only here), the kind to memory, the pose's two minima and four
//                                       counts into its row.
//   clearance_batch_decide_kernel       one lane per pose: step 2's last line into the row, then clearanceLoopStep -- the statements
//                                       clearanceLevels runs on the host: the status, whether the pose splits, its next run's length;
//                                       the call's two totals.
//   clearance_batch_flags_kernel        one lane per cell: the scan's 64-bit word (a cell that splits 1, a final 2^32; a split candidate
//                                       of a pose that does not split is a final).
//   rocprim::exclusive_scan             over the cells of all poses: both ranks of a cell in one scan.  The scan keeps pose order and
//                                       the order inside a run, so the next list is laid out like this one.
//   one read-back                       the totals: the next list's length and the level's finals.
//   clearance_batch_emit_kernel         children into the next list with their pose index, finals as (pose, blo); the first lane of a
//                                       pose's run writes where its next run starts.
//
// and at the end clearance_batch_finish_kernel counts, a lane a final, each pose's finals above and not above its hi; one read-back of
// the rows follows and the host finishes every struct with the single call's statements (clearanceResult).  Launches and read-backs per
// level do not depend on the number of poses.
// The per-pose reductions are integer atomics whose result does not depend on the order of execution: atomicMin on clearanceKey
// (clearance.hpp: the order of <, -0.0 and +0.0 equal), atomicMin on a position, atomicAdd on counts -- one atomic a wave where the
// wave's lanes share a pose.  The value kept is always a cell's own bit pattern, read back from the cell the position names; for the
// two minima of blo, where only a zero has two patterns, the first zero of the run is tracked as the single call's reduction keeps it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
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

constexpr uint32_t kNoPose = 0xFFFFFFFFu;

// a pose's row.  The level's reductions are reset by the decide kernel once it has used them.
struct ClearanceBatchPose {
    double best, bestVa;
    IntegrateCell bestCell;
    uint32_t hasWitness;
    unsigned long long candKey;    // the least clearanceKey(vb) of the level's candidates
    unsigned long long minKey[2];  // the least clearanceKey(blo) of the level's finals [0] and split candidates [1]
    uint32_t candPos;              // the least position in the run among the holders of candKey
    uint32_t zeroPos[2];           // the first final / split candidate of the run with blo == 0: its sign is the minimum's
    uint32_t count[4];             // by kind: kClearOutside .. kClearFinal
    uint32_t notFinite;
    uint32_t mode;                 // what emit does with the run: 0 nothing, 1 every survivor is final, 2 the split candidates split
    uint32_t start[2], len[2];     // the run of the list of level l at [l & 1]
    ClearanceLoop loop;
    unsigned long long finPruned, finOpen;  // the finish kernel's counts
};

struct ClearanceBatchTotals {
    unsigned long long next, finals;  // the next list's length and this level's new finals, over all poses
};

__device__ __forceinline__ void poseLevelReset(ClearanceBatchPose& P) {
    P.candKey = P.minKey[0] = P.minKey[1] = kClearanceNoKey;
    P.candPos = P.zeroPos[0] = P.zeroPos[1] = kClearanceNoPos;
    P.count[0] = P.count[1] = P.count[2] = P.count[3] = 0u;
}

// true if all 64 lanes hold the same pose (a lane past the list holds kNoPose: a ragged wave is not uniform).  Called by every lane.
__device__ __forceinline__ bool waveSharesPose(uint32_t p) { return __all(p == (uint32_t)__builtin_amdgcn_readfirstlane((int)p)) != 0; }

__device__ __forceinline__ unsigned long long waveMinKey(unsigned long long k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    return k;
}

// key into *slot of the lane's pose (kClearanceNoKey: the lane has none).  Called by every lane of the wave; uniform: waveSharesPose.
__device__ __forceinline__ void poseMinKey(bool uniform, unsigned long long* slot, unsigned long long key) {
    if (uniform) {
        key = waveMinKey(key);
        if ((threadIdx.x & 63u) == 0u && key != kClearanceNoKey) atomicMin(slot, key);
    } else if (key != kClearanceNoKey) {
        atomicMin(slot, key);
    }
}

// list 0 of every pose of the chunk, and the rows' first values
__global__ __launch_bounds__(kClrThreads) void clearance_batch_start_kernel(const IntegrateCell* __restrict__ leaves, uint32_t nLeaves, uint32_t nPoses,
                                                                            IntegrateCell* __restrict__ list, uint32_t* __restrict__ poseOf,
                                                                            ClearanceBatchPose* __restrict__ poses) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i < nLeaves * nPoses) {
        list[i] = leaves[i % nLeaves];
        poseOf[i] = i / nLeaves;
    }
    if (i < nPoses) {
        ClearanceBatchPose P{};
        P.best = boundsInf();
        poseLevelReset(P);
        P.start[0] = i * nLeaves, P.len[0] = nLeaves;
        clearanceLoopStart(P.loop);
        poses[i] = P;
    }
}

template <int MAXP>
__global__ __launch_bounds__(kClrThreads) void clearance_batch_bound_kernel(ClsTree tA, ClsTree tB, const PairArgs* __restrict__ args,
                                                                            const DeviceTables* __restrict__ T, IntegrateCell* __restrict__ list,
                                                                            const uint32_t* __restrict__ poseOf, uint32_t n, int level,
                                                                            double* __restrict__ blo, double* __restrict__ vb, double* __restrict__ va,
                                                                            ClearanceBatchPose* __restrict__ poses) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint32_t sFirst[kLevels * kClrThreads];
    __shared__ uint8_t sMask[kLevels * kClrThreads];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    LdsClrStack st{sFirst + threadIdx.x, sMask + threadIdx.x};
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    uint32_t p = kNoPose;
    unsigned long long key = kClearanceNoKey;
    if (i < n) {
        p = poseOf[i];
        const IntegrateCell c = list[i];
        bool finite = true;
        ClearanceCell o;
        clearanceCell(tA, tB, args[p], c, level, eval, st, &finite, o);
        list[i].cls = (uint8_t)o.clsA;
        blo[i] = o.blo, vb[i] = o.vb, va[i] = o.va;
        if (o.vb < boundsInf()) key = clearanceKey(o.vb);
        if (!finite) poses[p].notFinite = 1u;  // (every writer stores the same word)
    }
    const bool uniform = waveSharesPose(p);
    poseMinKey(uniform, p != kNoPose ? &poses[p].candKey : nullptr, key);
}

__global__ __launch_bounds__(kClrThreads) void clearance_batch_pick_kernel(const uint32_t* __restrict__ poseOf, const double* __restrict__ vb, uint32_t n,
                                                                           int par, ClearanceBatchPose* __restrict__ poses) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i >= n) return;
    const double v = vb[i];
    if (!(v < boundsInf())) return;
    ClearanceBatchPose& P = poses[poseOf[i]];
    if (clearanceKey(v) == P.candKey) atomicMin(&P.candPos, i - P.start[par]);
}

// best after step 2's last line, from the row as the pick kernel left it
__device__ __forceinline__ double poseBestNow(const ClearanceBatchPose& P, const double* __restrict__ vb, int par) {
    if (P.candPos == kClearanceNoPos) return P.best;
    const double v = vb[P.start[par] + P.candPos];
    return v < P.best ? v : P.best;
}

static_assert(kClearOutside == 0u && kClearPruned == 1u && kClearSplit == 2u && kClearFinal == 3u, "clearance_batch_prune_kernel counts by kind");

__global__ __launch_bounds__(kClrThreads) void clearance_batch_prune_kernel(const IntegrateCell* __restrict__ list, const uint32_t* __restrict__ poseOf,
                                                                            const double* __restrict__ blo, const double* __restrict__ vb, uint32_t n,
                                                                            uint32_t maxDepth, int par, uint8_t* __restrict__ kinds,
                                                                            ClearanceBatchPose* __restrict__ poses) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    uint32_t p = kNoPose, kind = 0xFFu;
    unsigned long long keyFinal = kClearanceNoKey, keySplit = kClearanceNoKey;
    if (i < n) {
        p = poseOf[i];
        ClearanceBatchPose& P = poses[p];
        const IntegrateCell c = list[i];
        const double b = blo[i];
        kind = clearanceKind(c.cls, b, poseBestNow(P, vb, par), c.depth, maxDepth);
        kinds[i] = (uint8_t)kind;
        if (kind == kClearFinal) keyFinal = clearanceKey(b);
        if (kind == kClearSplit) keySplit = clearanceKey(b);
        if ((kind == kClearFinal || kind == kClearSplit) && b == 0.0) atomicMin(&P.zeroPos[kind == kClearSplit ? 1 : 0], i - P.start[par]);
    }
    const bool uniform = waveSharesPose(p);
    ClearanceBatchPose* P = p != kNoPose ? &poses[p] : nullptr;
    poseMinKey(uniform, P ? &P->minKey[0] : nullptr, keyFinal);
    poseMinKey(uniform, P ? &P->minKey[1] : nullptr, keySplit);
    if (uniform) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
            if ((threadIdx.x & 63u) == 0u && c != 0u) atomicAdd(&P->count[k], c);
        }
    } else if (P) {
        atomicAdd(&P->count[kind], 1u);
    }
}

// a minimum of blo from its key: the key's double, and for a zero the pattern of the run's first zero of that kind
__device__ __forceinline__ double poseMinBlo(const ClearanceBatchPose& P, int which, const double* __restrict__ blo, int par) {
    const double v = clearanceKeyValue(P.minKey[which]);
    return v == 0.0 && P.zeroPos[which] != kClearanceNoPos ? blo[P.start[par] + P.zeroPos[which]] : v;
}

__global__ __launch_bounds__(kClrThreads) void clearance_batch_decide_kernel(const IntegrateCell* __restrict__ list, const double* __restrict__ blo,
                                                                             const double* __restrict__ vb, const double* __restrict__ va,
                                                                             uint32_t nPoses, int level, ClearanceArgs a,
                                                                             ClearanceBatchPose* __restrict__ poses,
                                                                             ClearanceBatchTotals* __restrict__ totals) {
    const uint32_t p = blockIdx.x * kClrThreads + threadIdx.x;
    if (p >= nPoses) return;
    ClearanceBatchPose& P = poses[p];
    const int par = level & 1;
    const uint32_t n = P.len[par];
    P.len[0] = P.len[1] = 0u, P.mode = 0u;  // (this level's run keeps its start for emit; the next run's length follows below)
    if (n == 0u) return;  // stopped at an earlier level
    clearanceLoopVisit(P.loop, level, n);
    if (P.notFinite != 0u) {
        P.loop.status = HPSDF_CLEARANCE_NOT_FINITE;
        return;
    }
    if (P.candPos != kClearanceNoPos) {  // step 2's last line
        const uint32_t at = P.start[par] + P.candPos;
        const double v = vb[at];
        if (v < P.best) P.best = v, P.bestVa = va[at], P.bestCell = list[at], P.hasWitness = 1u;
    }
    const uint32_t nSplit = P.count[kClearSplit], nFinal = P.count[kClearFinal];
    const int step = clearanceLoopStep(P.loop, a, P.best, poseMinBlo(P, 0, blo, par), poseMinBlo(P, 1, blo, par), P.count[kClearOutside],
                                       P.count[kClearPruned], nSplit, nFinal);
    poseLevelReset(P);
    if (step == kClearLoopEmpty) return;
    const bool split = step == kClearLoopSplit;
    P.mode = split ? 2u : 1u;
    P.len[par ^ 1] = split ? 8u * nSplit : 0u;
    if (split) atomicAdd(&totals->next, (unsigned long long)(8u * nSplit));
    const unsigned long long finals = split ? nFinal : nFinal + nSplit;
    if (finals != 0ull) atomicAdd(&totals->finals, finals);
}

__global__ __launch_bounds__(kClrThreads) void clearance_batch_flags_kernel(const uint32_t* __restrict__ poseOf, const uint8_t* __restrict__ kinds, uint32_t n,
                                                                            const ClearanceBatchPose* __restrict__ poses,
                                                                            unsigned long long* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t mode = poses[poseOf[i]].mode, kind = kinds[i];
    unsigned long long f = 0ull;
    if (mode != 0u && (kind == kClearSplit || kind == kClearFinal)) f = mode == 2u && kind == kClearSplit ? 1ull : 1ull << 32;
    flags[i] = f;
}

// ranks: the exclusive scan of flags over the whole list (low word: cells that split before this one, high word: finals)
__global__ __launch_bounds__(kClrThreads) void clearance_batch_emit_kernel(const IntegrateCell* __restrict__ list, const uint32_t* __restrict__ poseOf,
                                                                           const double* __restrict__ blo, uint32_t n, int par,
                                                                           const unsigned long long* __restrict__ flags,
                                                                           const unsigned long long* __restrict__ ranks,
                                                                           ClearanceBatchPose* __restrict__ poses, IntegrateCell* __restrict__ next,
                                                                           uint32_t* __restrict__ nextPose, uint32_t* __restrict__ finalPose,
                                                                           double* __restrict__ finalBlo) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = poseOf[i];
    const unsigned long long f = flags[i], r = ranks[i];
    const uint32_t rs = (uint32_t)r, rf = (uint32_t)(r >> 32);
    if (i == poses[p].start[par]) poses[p].start[par ^ 1] = 8u * rs;  // (the runs of the next list follow one another in pose order)
    if (f == 0ull) return;
    if (f == 1ull) {
        const IntegrateCell c = list[i];
        for (uint32_t ch = 0; ch < 8u; ++ch) next[8u * rs + ch] = integrateChild(c, ch), nextPose[8u * rs + ch] = p;
        return;
    }
    finalPose[rf] = p;
    finalBlo[rf] = blo[i];
}

// the end's filter of the finals, counted: blo > hi joins cells_pruned, the rest is cells_open
__global__ __launch_bounds__(kClrThreads) void clearance_batch_finish_kernel(const uint32_t* __restrict__ finalPose, const double* __restrict__ finalBlo,
                                                                             uint32_t n, ClearanceBatchPose* __restrict__ poses) {
    const uint32_t i = blockIdx.x * kClrThreads + threadIdx.x;
    if (i >= n) return;
    ClearanceBatchPose& P = poses[finalPose[i]];
    atomicAdd(finalBlo[i] > P.best ? &P.finPruned : &P.finOpen, 1ull);
}

constexpr int kChunkTooLarge = -1;  // runChunk: the chunk's next list does not fit the budget (no HPSDF status is negative)

struct DeviceClearanceBatch {
    hpsdf_ctx* ctx;
    const ClsTree& tA;
    const ClsTree& tB;
    int maxDegree;
    const IntegrateCell* dLeaves;
    uint32_t nLeaves;
    const double* posesIn;
    double isoA;
    uint32_t maxLeaves;
    const ClearanceArgs& a;
    uint32_t maxTotal;

    // grows an array of the pool to `need` elements, once the stream has passed every use of the old one
    template <class T>
    int fit(DevPool& pool, T*& ptr, size_t& cap, size_t need, const char* name) {
        if (need <= cap) return HPSDF_OK;
        if (ptr != nullptr) HPSDF_HIP(hipStreamSynchronize(ctx->stream));
        pool.release(ptr);
        SURF_ALLOC(pool, ptr, need * sizeof(T), name);
        cap = need;
        return HPSDF_OK;
    }

    // poses [first, first + count) from list 0 to the end -> res[first ..]; kChunkTooLarge: nothing was written, halve the chunk
    int runChunk(DevPool& pool, size_t first, uint32_t count, hpsdf_clearance* res) {
        hipStream_t s = ctx->stream;
        std::vector<PairArgs> hArgs(count);
        for (uint32_t p = 0; p < count; ++p) hArgs[p] = pairArgs(tA, HPSDF_PAIR_INTERSECTION, posesIn + 12 * (first + p), isoA, 0.0, maxLeaves);
        std::vector<ClearanceBatchPose> hPoses(count);
        PairArgs* dArgs = nullptr;
        ClearanceBatchPose* dPoses = nullptr;
        ClearanceBatchTotals* dTotals = nullptr;
        IntegrateCell* list[2] = {nullptr, nullptr};
        uint32_t* poseOf[2] = {nullptr, nullptr};
        size_t listCap[2] = {0, 0}, poseCap[2] = {0, 0};
        double *blo = nullptr, *vb = nullptr, *va = nullptr;
        uint8_t* kinds = nullptr;
        unsigned long long *flags = nullptr, *ranks = nullptr;
        size_t bloCap = 0, vbCap = 0, vaCap = 0, kindsCap = 0, flagsCap = 0, ranksCap = 0;
        std::vector<std::pair<uint32_t*, double*>> finals;  // a pair of arrays a level, with their length
        std::vector<uint32_t> finalsLen;
        uint32_t n = nLeaves * count;
        SURF_ALLOC(pool, dArgs, (size_t)count * sizeof(PairArgs), "pose arguments");
        SURF_ALLOC(pool, dPoses, (size_t)count * sizeof(ClearanceBatchPose), "pose rows");
        SURF_ALLOC(pool, dTotals, sizeof(ClearanceBatchTotals), "totals");
        HPSDF_HIP(hipMemcpyAsync(dArgs, hArgs.data(), (size_t)count * sizeof(PairArgs), hipMemcpyHostToDevice, s));
        if (const int rc = fit(pool, list[0], listCap[0], n, "list 0")) return rc;
        if (const int rc = fit(pool, poseOf[0], poseCap[0], n, "list 0")) return rc;
        hipLaunchKernelGGL(clearance_batch_start_kernel, dim3(clrBlocks(n > count ? n : count)), dim3(kClrThreads), 0, s, dLeaves, nLeaves, count, list[0],
                           poseOf[0], dPoses);
        HPSDF_HIP(hipGetLastError());
        for (int level = 0; n != 0; ++level) {
            const int par = level & 1;
            const uint32_t nb = clrBlocks(n);
            if (const int rc = fit(pool, blo, bloCap, n, "cell bounds")) return rc;
            if (const int rc = fit(pool, vb, vbCap, n, "candidates")) return rc;
            if (const int rc = fit(pool, va, vaCap, n, "candidates")) return rc;
            if (const int rc = fit(pool, kinds, kindsCap, n, "kinds")) return rc;
            if (const int rc = fit(pool, flags, flagsCap, n, "flags")) return rc;
            if (const int rc = fit(pool, ranks, ranksCap, n, "ranks")) return rc;
            IntegrateCell* cur = list[par];
            uint32_t* curPose = poseOf[par];
            forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
                constexpr int MAXP = decltype(P)::value;
                hipLaunchKernelGGL((clearance_batch_bound_kernel<MAXP>), dim3(nb), dim3(kClrThreads), 0, s, tA, tB, dArgs, ctx->dTables, cur, curPose, n,
                                   level, blo, vb, va, dPoses);
            });
            HPSDF_HIP(hipGetLastError());
            hipLaunchKernelGGL(clearance_batch_pick_kernel, dim3(nb), dim3(kClrThreads), 0, s, curPose, vb, n, par, dPoses);
            HPSDF_HIP(hipGetLastError());
            hipLaunchKernelGGL(clearance_batch_prune_kernel, dim3(nb), dim3(kClrThreads), 0, s, cur, curPose, blo, vb, n, a.depth, par, kinds, dPoses);
            HPSDF_HIP(hipGetLastError());
            HPSDF_HIP(hipMemsetAsync(dTotals, 0, sizeof(ClearanceBatchTotals), s));
            hipLaunchKernelGGL(clearance_batch_decide_kernel, dim3(clrBlocks(count)), dim3(kClrThreads), 0, s, cur, blo, vb, va, count, level, a, dPoses,
                               dTotals);
            HPSDF_HIP(hipGetLastError());
            hipLaunchKernelGGL(clearance_batch_flags_kernel, dim3(nb), dim3(kClrThreads), 0, s, curPose, kinds, n, dPoses, flags);
            HPSDF_HIP(hipGetLastError());
            void* tmp = nullptr;
            size_t bytes = 0;
            const unsigned long long* in = flags;
            unsigned long long* out = ranks;
            if (const int rc = withTemp(pool, "rocprim::exclusive_scan", "scan storage", tmp, bytes, [=](void* q, size_t& b) {
                    return rocprim::exclusive_scan(q, b, in, out, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), s);
                }))
                return rc;
            ClearanceBatchTotals t{};
            HPSDF_HIP(hipMemcpyAsync(&t, dTotals, sizeof t, hipMemcpyDeviceToHost, s));
            HPSDF_HIP(hipStreamSynchronize(s));
            pool.release(tmp);
            if (t.next > maxTotal && count > 1u) return kChunkTooLarge;
            uint32_t* fp = nullptr;
            double* fb = nullptr;
            if (t.finals != 0ull) {
                SURF_ALLOC(pool, fp, (size_t)t.finals * sizeof(uint32_t), "final cells");
                SURF_ALLOC(pool, fb, (size_t)t.finals * sizeof(double), "final bounds");
                finals.emplace_back(fp, fb);
                finalsLen.push_back((uint32_t)t.finals);
            }
            if (const int rc = fit(pool, list[par ^ 1], listCap[par ^ 1], (size_t)t.next, "the next list")) return rc;
            if (const int rc = fit(pool, poseOf[par ^ 1], poseCap[par ^ 1], (size_t)t.next, "the next list")) return rc;
            if (t.next != 0ull || t.finals != 0ull) {
                hipLaunchKernelGGL(clearance_batch_emit_kernel, dim3(nb), dim3(kClrThreads), 0, s, cur, curPose, blo, n, par, flags, ranks, dPoses,
                                   list[par ^ 1], poseOf[par ^ 1], fp, fb);
                HPSDF_HIP(hipGetLastError());
            }
            n = (uint32_t)t.next;
        }
        for (size_t l = 0; l < finals.size(); ++l) {
            hipLaunchKernelGGL(clearance_batch_finish_kernel, dim3(clrBlocks(finalsLen[l])), dim3(kClrThreads), 0, s, finals[l].first, finals[l].second,
                               finalsLen[l], dPoses);
            HPSDF_HIP(hipGetLastError());
        }
        HPSDF_HIP(hipMemcpyAsync(hPoses.data(), dPoses, (size_t)count * sizeof(ClearanceBatchPose), hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipStreamSynchronize(s));
        for (uint32_t p = 0; p < count; ++p) {
            const ClearanceBatchPose& P = hPoses[p];
            hpsdf_clearance& r = res[first + p];
            if (P.loop.status == HPSDF_CLEARANCE_NOT_FINITE) {
                clearanceNotFinite(P.loop.levels, &r);
                continue;
            }
            // the witness's point and image are made on the host from its cell by the kernels' statements: no tree is read for them
            clearanceResult(tA, hArgs[p], P.loop, P.best, P.bestVa, P.bestCell, P.hasWitness, r);
            if (P.loop.status != HPSDF_CLEARANCE_EMPTY) r.cells_pruned += P.finPruned, r.cells_open = P.finOpen;
        }
        return HPSDF_OK;
    }
};

}  // namespace

// ClearanceBatch over two device trees of one device (the trees, dLeaves and maxDegree as for clearanceOnDevice): the poses in chunks
// whose lists 0 fit maxTotalCells together; a chunk that outgrows it is halved and its halves start again.  A pose's result does not
// depend on its chunk.  Synchronises the context stream before it returns; frees everything it took, whatever happens; writes `out`
// only when every pose succeeded.
int clearanceBatchOnDevice(hpsdf_ctx* ctx, const ClsTree& ctA, const ClsTree& ctB, int maxDegree, const IntegrateCell* dLeaves, uint32_t nLeaves,
                           const double* poses, size_t n, double isoA, uint32_t maxLeaves, const ClearanceArgs& a, uint32_t maxTotalCells,
                           hpsdf_clearance* out) {
    DeviceClearanceBatch B{ctx, ctA, ctB, maxDegree, dLeaves, nLeaves, poses, isoA, maxLeaves, a, maxTotalCells};
    std::vector<hpsdf_clearance> res(n);
    const size_t most = nLeaves != 0u && maxTotalCells / nLeaves > 0u ? maxTotalCells / nLeaves : 1u;  // poses whose lists 0 fit together
    std::vector<std::pair<size_t, size_t>> todo;  // (first, count), the next chunk last
    for (size_t first = n; first != 0;) {
        const size_t count = (first - 1) % most + 1;  // (the short chunk is the last one)
        first -= count;
        todo.emplace_back(first, count);
    }
    while (!todo.empty()) {
        const std::pair<size_t, size_t> c = todo.back();
        todo.pop_back();
        DevPool pool{"hpsdf_clearance_batch_device"};  // the chunk's device memory: freed at the end of this pass, whatever happens
        const int rc = B.runChunk(pool, c.first, (uint32_t)c.second, res.data());
        if (rc == kChunkTooLarge) {
            const size_t half = c.second / 2;
            todo.emplace_back(c.first + half, c.second - half);
            todo.emplace_back(c.first, half);
            continue;
        }
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call runs on when its arrays go)
            return rc;
        }
    }
    std::memcpy(out, res.data(), n * sizeof(hpsdf_clearance));
    return HPSDF_OK;
}

}  // namespace hpsdf
