// What the device frontier's kernels (frontier.hip) and Create's driver on the host (frontier_build.cpp) share: the state both
// sides address, the shape rules both sides evaluate, and the launchers through which the driver reaches the kernels.  Plain C++
// as well as HIP: no device-only code here.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "device_types.hpp"
#include "launch.hpp"
#include "tables.hpp"

namespace hpsdf {

constexpr uint32_t kFrJobs = 4096;  // largest batch: K <= 4096, and round 0 is the 4096 depth-4 cells
constexpr uint32_t kFrTasks = 9 * kFrJobs;
constexpr int kFrSegs = 10;         // degrees 2..11: the first fit and at most nine P-refinements
constexpr int kFrDepths = kMaxDepth + 2;
constexpr int kFrClasses = 2 * (kMaxDegree + 1) * kFrDepths;  // (degree, from scratch | incremental, depth)
constexpr uint64_t kNotQueued = ~0ull;
constexpr uint64_t kOffMask = (1ull << 56) - 1;  // a segment's arena offset; the bits above hold the rank that owns it
// Multi-rank builds: the last double of a rank's part of errs is its STATUS for the round's exchange.  A healthy rank zeroes it
// (fr_init_kernel, the round kernel's leader or fr_batch_kernel); a rank whose share of the round failed on the host (device memory) sets it to all ones and
// enters the exchange all the same; the round kernel's leader finds it (frPeerCheck) and every rank leaves with an error instead of
// waiting in a later collective for a rank that has gone.
constexpr uint32_t kFrStatusPad = 8;
constexpr uint32_t kFrInlineNodes = 131072;  // trees up to here are selected by the closing workgroup itself (128 passes of 1024 lanes; its bitmap
                                             // holds 262 144 nodes.  65 536 sent union3 @ 4.5e-9, K = 4096 -- 58 k nodes + 32 k of room for a round -- to the
                                             // grid selection in its last rounds: 5.8 ms against 4.5)

struct FrHdr {
    uint32_t nNodes, nQueued, nJobs, done;
    uint32_t round, maxDegree, maxDepth, overflow;
    uint32_t nTasks, nBlocks, takenCount, candCount;
    uint32_t above;   // selection, level 0: queued nodes in the exponent bins above the threshold bin t1
    int32_t t1;       // (-1: the whole frontier is the batch); both are left by the previous round's update kernel
    uint32_t nLeaves, arrive;
    uint32_t degBlocks[13][2];  // {first block, count} per degree: the range a fit launch walks
    uint32_t degTasks[13][2];   // {first task, count} per degree: the range a mesh-sampler launch walks
    uint32_t lowTasks[13][2];   // {first task, count} per degree: the from-scratch fits that are split (FitBlock::split), i.e. the
                                // range fit_mfma_low_kernel walks for the rows below the top degree
    uint64_t arenaUsed, sampleUsed, nCoeffs, pad1;
    uint64_t jobs, pRefines, hRefines, dropped, fits, samples;
    uint64_t splitFits;   // from-scratch fits whose lower rows came from the split's second kernel (hpsdf_build_stats::split_fits)
    uint32_t splitRound, padR;  // FrDev::splitFit if the round being prepared splits its from-scratch fits, else 0 (decided by the batch)
    uint64_t roundBase, partStride;  // FrDev::replica: the round's fits write arena rows [roundBase + r partStride, + partStride) on rank r
    double total, target;
    // staging between the decide and update kernels of a round
    uint32_t rP, rH, rD, rMaxDeg;
    uint32_t rOps, rPad;
    uint32_t sliceFirst[9];  // multi-rank: rank r computes jobs [sliceFirst[r], sliceFirst[r + 1]) of the round
    uint32_t padS;
    uint64_t packCount[8];   // multi-rank: coefficients rank r contributes to the packed store
    uint64_t dbg[24];  // phase time stamps (s_memtime) of the one-workgroup kernels, read under HPSDF_TRACE
    int64_t rCoeffDelta;
    double rTotal;
    uint32_t opsArrive, stuck;  // fr_round_kernel: update workgroups whose operands are written; a wait that ran out (never, by construction)
    uint32_t chainStamp;  // round + 1 once rTotal holds that round's running total
    uint32_t landed;      // (mirror only) the build's stamp, written when round 0's closing launch starts: the fit before it has finished, so
                          // the rows it wrote into pinned host memory are there
    uint32_t stored[2];   // (mirror only) the build's stamp once fr_store_kernel's node array / coefficients are in pinned host memory
    uint32_t storeArrive[2];  // workgroups of fr_store_kernel that have finished a phase
    uint32_t hist1[2048];  // queued nodes per exponent bin (kept by update / batch)
    uint32_t hist2[2048];  // level-1 digits of the candidates of the current selection (grid selection only)
    uint64_t agg[kFrJobs / 128];  // fr_round_kernel: per update workgroup {round stamp, splitting jobs << 16 | P jobs}
};
constexpr size_t kFrHdrCopyBytes = offsetof(FrHdr, hist1);

struct FrRound {  // shape classes of the current round (written by fr_batch_kernel, read by fr_tasks_kernel)
    uint32_t cCount[kFrClasses], cFirst[kFrClasses], cCursor[kFrClasses], cBlockFirst[kFrClasses], cBlocks[kFrClasses];
    uint64_t cArena[kFrClasses], cSample[kFrClasses];
    uint64_t cArenaO[8][kFrClasses];  // FrDev::replica: arena rows before class c within owner o's part of the round
    uint8_t cG[kFrClasses], cPlanes[kFrClasses];
    uint64_t arenaBase;
};

struct FrDev {
    FrHdr* hdr;
    FrHdr* hostHdr;  // the header's mirror in pinned host memory, as the device addresses it
    FrRound* rnd;
    hpsdf_node* nodes;
    uint64_t* qErr;     // bit pattern of the queued error; kNotQueued = not in the frontier
    uint32_t* parent;
    uint64_t* segOff;   // [node][kFrSegs] arena offsets (doubles)
    uint8_t* segFirst;  // degree of the node's first segment
    uint32_t* sub;      // coefficients below every interior node (kept incrementally from round 1 on)
    uint32_t* taken;    // selection: nodes taken so far (unordered)
    uint32_t* candA;
    uint32_t* candB;
    const uint32_t* batchIdx;  // the round's jobs in node-index order (round 0: the template's)
    const double* batchErr;
    const uint64_t* jobP;      // per job: arena offset of the P result / of the first H child
    const uint64_t* jobH;
    uint32_t* wBatchIdx;       // the same buffers, writable (rounds > 0)
    double* wBatchErr;
    uint64_t* wJobP;
    uint64_t* wJobH;
    double* ops;               // the round's additions to the running total, densely, in job order
    uint32_t* jobRecA;         // per job of the round being opened, for fr_emit_kernel: H slot | P slot << 16 | degree << 28
    uint16_t* jobRecB;         //   coarse | ours << 1 | owner << 2 | depth << 5
    FitTask* tasks;
    FitBlock* blocks;
    double* errs;       // [jobs][9]
    double* store;      // the finished block's coefficients and, behind them, its node array: pinned host memory as the device addresses it
    const double* arena;
    uint32_t nodeCap, K;
    // multi-rank builds (world > 1): this rank fits a cost-balanced slice of every round's jobs
    int32_t rank, world;
    uint32_t errStride;    // doubles per rank in errs: rank r's slice sits at errs + r * errStride (all-gathered in place)
    uint32_t errStrideNext;  // ... in the round being prepared (round 0 exchanges 4096 jobs' errors, later rounds K)
    uint8_t* jobOwner;     // per job: the rank that fits it
    uint32_t* packPos;     // [node][kFrSegs]: where the segment sits in its owner's pack buffer
    double* pack;          // [world][packStride] all-gathered pack buffers (this rank writes its own)
    uint64_t packStride;
    int32_t fastFit;       // degrees >= 4 fitted by fit_mfma.hip: 16 cells per workgroup
    int32_t splitFit;      // 0, or the lowest degree (.. 11) whose from-scratch fits are split: top-degree rows exact, the rest by fit_low_kernel.
                           // Whether a round does split is the batch's decision (FrHdr::splitRound), by the host scheduler's rule
    uint64_t sampleCap;    // doubles the sample buffer holds (the split's hand-over needs the round's samples to fit)
    // nearness weighting (Octree.cpp:1071-1092, 1209-1247): a fit keeps ONE full coefficient array (an incremental fit
    // carries the old rows over, :847), fit_weight_kernel leaves |mean FApprox| of every fit in `means`, the host turns
    // the means into weights with its libm (pow / exp: what the oracle calls) and fr_weigh_kernel scales the errors
    uint32_t buildStamp;  // a number of the build (FrHdr::landed)
    uint32_t stamps;      // HPSDF_TRACE: the one-workgroup kernels leave their phases' times in FrHdr::dbg (a store a phase, and the next barrier waits for it)
    double target;         // targetErrorThreshold of the build (the header is initialised before the build is known: FrontierWorkspace::clean)
    int32_t weighted;
    // Weighted builds on several ranks: every rank's arena is a REPLICA.  An incremental weighted fit carries the cell's previous rows
    // over (:847), and those may have been fitted anywhere -- so a round's fits are laid out owner by owner at the same offsets on every
    // rank (FrHdr::roundBase / partStride), every rank fills its own part, and ONE in-place all-gather of the round's part of the arena
    // (beside the errors') leaves every rank with every row.  Segments then need no owner, the packed store no exchange of its own.
    int32_t replica;
    double* means;          // [jobs][9], pinned host memory as the device addresses it (written by fit_weight_kernel)
    const double* weights;  // [jobs][9], pinned host memory as the device addresses it (written by the host)
    uint32_t* hostFlag;     // pinned: {jobs of the round, stamp}: "the means are there"
};

__host__ __device__ inline uint32_t frCoef(int p) { return p == 6 ? 83u : (uint32_t)((p + 1) * (p + 2) * (p + 3) / 6); }
__host__ __device__ inline int frClass(int degree, bool incr, int depth) { return (2 * degree + (incr ? 1 : 0)) * kFrDepths + depth; }
__host__ __device__ inline size_t frLds(int degree, int g, int planes) {  // = fitLdsBytes (fit.hip)
    const size_t nq = 4 * (size_t)degree + 1;
    return ((size_t)(degree + 1) * nq + 2 * nq + 8 * (size_t)g + (size_t)g * planes * nq * nq) * sizeof(double);
}
// workgroup shape of `count` fits of one class: what fitShape (fit.hip) gives an unweighted, sampled-or-analytic fit
// splitFit: 0 = off, else the lowest degree whose from-scratch fits are split (the context's splitMinDegree)
constexpr size_t kFrFitLdsCap = 45 * 1024;
__host__ __device__ inline bool frSplit(int splitFit, int degree, bool incr) { return splitFit > 0 && !incr && degree >= splitFit && degree <= 11; }
__host__ __device__ inline void frShape(int degree, bool incr, uint32_t count, int* cells, int* planes, bool fast = false, bool weighted = false,
                                        int split = 0) {
    if (fast && degree >= 4 && degree <= 11) {  // the matrix-core fit: one workgroup = one tile of 16 cells
        *cells = kMfmaCells, *planes = 1;
        return;
    }
    if (frSplit(split, degree, incr)) incr = true;  // the exact kernel fits the top-degree rows only: the shape of an incremental fit
    const int nrows = incr ? (int)(frCoef(degree) - frCoef(degree - 1)) : (int)frCoef(degree);
    int gmax = nrows > kFitBlockThreads ? 1 : kFitBlockThreads / nrows;
    // (45 KB of dynamic LDS + the fit kernel's 7 KB of static keep three workgroups on a CU at every degree.  Up to kFitMaxLdsBytes the
    // incremental fits of degrees 6, 8, 9 and 11 stacked one or two cells more -- and a round launched for "one degree more than the
    // host knows" ran two workgroups a CU: 238 us instead of 194)
    while (gmax > 1 && frLds(degree, gmax, 1) > (weighted ? kFitMaxLdsBytes : kFrFitLdsCap)) --gmax;
    uint32_t spread = (count + 511u) / 512u;
    int cap = gmax;
    if (degree == 2) {  // as fitShape: measured best for degree 2
        if (count <= 4096u) spread = (count + 1023u) / 1024u;
        cap = gmax < 16 ? gmax : 16;
    }
    int g = (int)(spread < 1u ? 1u : spread);
    g = g < cap ? g : cap;
    const int nq = 4 * degree + 1;
    int pl = nq;
    while (pl > 1 && frLds(degree, g, pl) > kFitChunkLdsBytes) --pl;
    if (weighted) {  // as fitShape: the sample region is reused for the full coefficient array + 100 FApprox values of every cell
        const int need = (int)frCoef(degree) + 100;
        const int minPlanes = (need + nq * nq - 1) / (nq * nq);
        const int want = nq < minPlanes ? nq : minPlanes;
        pl = pl > want ? pl : want;
        while (g > 1 && frLds(degree, g, pl) > kFitMaxLdsBytes) --g;
    }
    *cells = g;
    *planes = pl;
}

// what fr_init_kernel copies: the uniformly refined tree and round 0 (FrontierWorkspace::tmpl, FrontierBuild::T0)
struct FrTemplate {
    const hpsdf_node* nodes;
    const uint32_t* parent;
    const uint32_t* sub;
    uint32_t nNodes, nLeaves, nTasks, nBlocks;  // nTasks / nBlocks / arenaRows / samples: this rank's share of round 0
    uint64_t arenaRows, samples;
    uint32_t sliceFirst[9];
};

// One launcher per kernel of frontier.hip, in the kernels' order.  The caller names the problem's size (jobs, nodes); grid and
// workgroup are the kernel's business and are worked out beside it.  Each returns hipGetLastError().
hipError_t frLaunchSelect(hipStream_t stream, const FrDev& d, uint32_t nodes);
hipError_t frLaunchEmit(hipStream_t stream, const FrDev& d, uint32_t jobs);
hipError_t frLaunchBatch(hipStream_t stream, const FrDev& d);
hipError_t frLaunchTasks(hipStream_t stream, const FrDev& d, uint32_t jobs);
hipError_t frLaunchRound(hipStream_t stream, const FrDev& d, uint32_t jobs, int flags);  // jobs of the round being closed
// (diagnostics: the running total's chain alone, on the caller's operands -- ops[n], or errs[9 n] and batchErr[n] when round0; hdr: sizeof(FrHdr) bytes)
hipError_t frLaunchRunningTotal(hipStream_t stream, FrHdr* hdr, const double* ops, const double* errs, const double* batchErr, double total0,
                                uint32_t n, bool round0, bool allWaves, double* out);
hipError_t frLaunchSubtree(hipStream_t stream, const FrDev& d, uint32_t nodes);
hipError_t frLaunchStore(hipStream_t stream, const FrDev& d, uint32_t nodes);
hipError_t frLaunchPackPos(hipStream_t stream, const FrDev& d);
hipError_t frLaunchPack(hipStream_t stream, const FrDev& d, uint32_t nodes);
hipError_t frLaunchMeansDone(hipStream_t stream, const FrDev& d, uint32_t stamp);
hipError_t frLaunchWeigh(hipStream_t stream, const FrDev& d, uint32_t stride, uint32_t base, uint32_t jobs);  // nine error slots a job from `base`
hipError_t frLaunchInit(hipStream_t stream, const FrDev& d, const FrTemplate& t);

}  // namespace hpsdf
