// Create's driver for the device frontier, on the host: which builds take it (frontierEligible) and the build itself
// (frontierCreate) -- per round a fixed sequence of launches through frontier.hip's launchers (frontier_dev.hpp) and one look at
// the header's mirror.  What the kernels do is said in frontier.hip; the round schedule is DESIGN.md section 3.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "block.hpp"
#include "builder.hpp"
#include "frontier.hpp"
#include "frontier_dev.hpp"
#include "frontier_workspace.hpp"
#include "launch.hpp"
#include "runtime.hpp"

namespace hpsdf {

static inline void frCpuRelax() {  // the host's spin on the header mirror
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#endif
}

bool frontierEligible(const hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, uint64_t K) {
    if (const char* e = std::getenv("HPSDF_HOST_FRONTIER"))
        if (e[0] == '1') return false;
    if (cfg->weighting_type > 2) return false;    // (unknown weighting: the host scheduler reports it)
    if (cfg->enable_logging) return false;        // the per-job log line is printed by the host scheduler
    const hpsdf_field* in = innermost(field);
    if (!in || (in->kind != kHostAnalytic && in->kind != kHostMesh)) return false;  // callbacks are sampled by host threads
    if (in->kind == kHostMesh) {
        const char* e = std::getenv("HPSDF_MESH_FUSED");
        if (e && e[0] == '1') return false;
        if (meshFaceRuleReference(ctx)) return false;  // (the sampler's shared traversal assumes the default face rule: builder.cpp fits with the per-point one)
    }
    const uint64_t k = K ? K : HPSDF_DEFAULT_JOBS_PER_ROUND;
    return k <= kFrJobs;
}

// A launch that failed (LDS over-subscription, a grid beyond the limits) used to surface a round later as "a round ended without
// advancing": every launch of the build loop reports its own failure at once.  (kernel: the name a message carries; launcher: its
// frLaunch* of frontier_dev.hpp, called with the stream and the arguments that follow)
#define FR_LAUNCH(kernel, launcher, stream, ...)                                            \
    do {                                                                                    \
        const hipError_t le_ = launcher(stream, __VA_ARGS__);                               \
        if (le_ != hipSuccess) return ::hpsdf::hipFail(le_, "launch of " #kernel);          \
        if (frSyncEveryLaunch()) {                                                          \
            std::fprintf(stderr, "[frontier] " #kernel " ...");                             \
            const hipError_t se_ = hipStreamSynchronize(stream);                            \
            std::fprintf(stderr, " %s\n", hipGetErrorString(se_));                          \
        }                                                                                   \
    } while (0)
static bool frSyncEveryLaunch() {  // HPSDF_FRONTIER_SYNC=1: a fault names its kernel (diagnostic; the host's waits then find every round closed)
    static const bool on = std::getenv("HPSDF_FRONTIER_SYNC") != nullptr;
    return on;
}

// ---------------------------------------------------------------------------------------------------------------------
// Create's driver: what the steps of a build share (file-level rules, the failure protocol, FrontierBuild), then the steps
// ---------------------------------------------------------------------------------------------------------------------
namespace {

inline double frNow() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The device tells the host that something is there by writing a word of pinned memory behind a system-scope fence.  Watching that
// word costs ~3 us; waking up from hipStreamSynchronize ~20.  Watches for `microseconds` and says whether the word arrived: what a
// caller falls back on when it did not (the ordinary wait, as a rule) and its acquire fence are the caller's.
inline bool watchWord(const volatile uint32_t* word, uint32_t want, double microseconds) {
    const double limit = frNow() + microseconds;
    while (*word != want && frNow() < limit) frCpuRelax();
    return *word == want;
}

// launch-time LDS of a fit launch of `deg`: the largest shape the device may pick
std::vector<size_t> makeLdsTable(bool w) {
    std::vector<size_t> t(kMaxDegree + 1, 0);
    for (int deg = 1; deg <= kMaxDegree; ++deg)
        for (int incr = 0; incr < 2; ++incr) {
            int g, pl;
            frShape(deg, incr != 0, 1u << 20, &g, &pl, false, w);  // g = the class's largest
            for (int gg = 1; gg <= g; ++gg) {
                const int nq = 4 * deg + 1;
                int pp = nq;
                while (pp > 1 && frLds(deg, gg, pp) > kFitChunkLdsBytes) --pp;
                if (w) {  // frShape's weighted adjustment
                    const int minPlanes = ((int)frCoef(deg) + 100 + nq * nq - 1) / (nq * nq);
                    pp = std::max(pp, std::min(nq, minPlanes));
                    if (gg > 1 && frLds(deg, gg, pp) > kFitMaxLdsBytes) continue;  // (frShape stacks fewer cells)
                }
                t[deg] = std::max(t[deg], frLds(deg, gg, pp));
            }
        }
    return t;
}
const std::vector<size_t>& fitLdsTable(bool weighted) {
    static const std::vector<size_t> fitLdsPlain = makeLdsTable(false), fitLdsWeighted = makeLdsTable(true);
    return weighted ? fitLdsWeighted : fitLdsPlain;
}
uint64_t rowsPerJob(int pmax) {  // arena rows one job can need when no leaf exceeds degree pmax
    const int p = std::min(pmax, kMaxDegree - 1);
    return (uint64_t)8 * frCoef(p) + frCoef(std::min(p + 1, kMaxDegree));
}
uint64_t samplesPerJob(int pmax) {
    const uint64_t a = 4 * (uint64_t)std::min(pmax, kMaxDegree - 1) + 1, b = a + 4;
    return 8 * a * a * a + b * b * b;
}

// Round 0 on several ranks: rank r fits cells [ends[r], ends[r + 1]) of the template's nLeaves.  Equal costs, so the slices end
// where the scheduler's rule puts them (builderSelect: the first i with i c >= total (r + 1) / world); ends beyond `world` are nLeaves.
// Depends on the template and the world size alone, so it is known before anything can fail.
void round0SliceEnds(uint32_t nLeaves, int world, uint32_t ends[9]) {
    ends[0] = 0;
    for (int r = 1; r < 9; ++r) ends[r] = nLeaves;
    const uint64_t c = (uint64_t)frCoef(2) * 729ull, total = c * nLeaves;
    uint32_t start = 0;
    for (int r = 0; r < world; ++r) {
        uint32_t end = nLeaves;
        if (r + 1 < world) {
            const uint64_t target = total * (uint64_t)(r + 1) / (uint64_t)world;
            end = (uint32_t)((target + c - 1) / c);
            end = std::min(std::max(end, start), nLeaves);
        }
        ends[r + 1] = end;
        start = end;
    }
}
// replica: doubles per rank in round 0's part of the arena (rank r's cells at r x this -- equal parts for the in-place all-gather)
uint64_t round0PartRows(const uint32_t ends[9], int world) {
    uint32_t maxCount = 1;
    for (int r = 0; r < world; ++r) maxCount = std::max(maxCount, ends[r + 1] - ends[r]);
    return ((uint64_t)maxCount * frCoef(2) + 15ull) & ~15ull;
}

void fillStats(const FrHdr* hh, uint64_t nNodes, uint64_t nCoeffs, int fitMode, hpsdf_build_stats* stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->rounds = hh->round, stats->jobs = hh->jobs, stats->p_refines = hh->pRefines, stats->h_refines = hh->hRefines;
    stats->dropped = hh->dropped, stats->fits = hh->fits, stats->samples = hh->samples;
    stats->n_nodes = nNodes, stats->n_leaves = hh->nLeaves, stats->n_coeffs = nCoeffs, stats->total_error = hh->total;
    stats->fit_mode = (uint64_t)fitMode, stats->split_fits = hh->splitFits, stats->device_frontier = 1;
}

// Several ranks: which exchanges the other ranks enter next.  If this rank's share fails while one is pending, it still enters it
// -- with its status slot set (kFrStatusPad) -- before it returns its error: the others then leave with HPSDF_ERR_STATE instead of
// waiting for a rank that has gone (FrontierBuild::leaveAfterFailure).
struct PendingExchange {
    enum Errors { kNone, kRound0, kLaterRound } errors = kNone;
    uint32_t errStride = 0;  // of that exchange: where this rank leaves its status
    // replica: the round's part of the arena while its exchange is still to come -- a failing rank enters it too, so round 0's part is
    // known before anything can fail.  Kept as an OFFSET into the arena (doubles) and a size: the arena can move between the moment
    // the part is known and the moment a failure sends this rank into the exchange (ensureArena reallocates), and a pointer taken
    // earlier would then name freed memory.
    bool rows = false;
    uint64_t rowsOff = 0;
    size_t rowsBytes = 0;

    void round0Begins(uint32_t stride0) { errors = kRound0, errStride = stride0; }
    void rowsAt(uint64_t off, size_t bytes) { rows = true, rowsOff = off, rowsBytes = bytes; }  // (round 0, the header, the batch kernel)
    void rowsEntered() { rows = false; }  // (a gather that fails is the callback's failure, not a reason to enter it again)
    void afterRound0Exchanges(uint32_t strideK) { errors = kNone, errStride = strideK; }
    void afterHeaderRead() { errors = kLaterRound; }
    void errorsExchanged() { errors = kNone; }
};

// One Create on the device frontier: what its steps share, and the steps.  run() is the build; a failure goes through
// leaveAfterFailure().  Every step returns a status, FR_LAUNCH and HPSDF_HIP return from the step they are used in.
struct FrontierBuild {
    hpsdf_ctx* const ctx;
    FrontierWorkspace* const ws;
    const hpsdf_config cfg;  // (the copy that goes into the block)
    const hpsdf_field* const field;
    void** const block;
    size_t* const size;
    hpsdf_build_stats* const stats;
    const int rank, world;
    const hpsdf_allgather_fn gather;
    void* const gatherUser;
    const bool trace;
    const double t0;
    // what follows from the arguments
    const hipStream_t s;
    const uint32_t Kj;
    // (replica: on several ranks a weighted incremental fit needs the node's previous rows, which another rank may have fitted: the
    // arenas are replicas of each other then -- FrDev::replica)
    const bool weighted, replica, mesh, splitMode;
    const uint32_t stride0, strideK;  // doubles per rank in errs, round 0 and later (at most K jobs: smaller parts to all-gather than round 0's 4096)
    const std::vector<size_t>& fitLds;
    FrDev& d;
    const FrTemplate& T;
    const FrHdr* const hh;
    uint32_t inlineNodes = kFrInlineNodes;  // trees up to here are selected by the closing launch itself, larger ones on the grid
    FieldDev fd;
    RootMap rm;
#ifdef HPSDF_TEST_HOOKS  // (lib/libhpsdf_hooks.so, built for tests/: the production library does not look at the variable)
    const char* const injected = std::getenv("HPSDF_TEST_FAIL_RANK");  // "<rank>:<round>"
#else
    static constexpr const char* injected = nullptr;  // (the statements that look at it fold away: the production library holds no trace of the hook)
#endif
    PendingExchange pending;
    // round 0's plan: this rank's share when there are several
    FrTemplate T0{};
    const FitTask* r0Tasks = nullptr;
    const FitBlock* r0Blocks = nullptr;
    const uint64_t* r0JobP = nullptr;
    size_t r0Lds = 0;
    uint64_t part0 = 0;  // replica: doubles per rank in round 0's part of the arena
    // the rounds
    int rounds = 0;  // rounds the host has seen closed
    uint32_t knownNodes = 0, knownMaxDeg = 2;
    uint64_t knownArena = 0;
    bool splitOpen = false, samplesTooLarge = false;  // of the round that the next closing launch opens (prepareNext)
    uint64_t measuredLimit = 0;  // (hpsdf_ctx_set_build_limits' default, measured at most once per Create: checkBuildLimits)
    // the round being closed, from closeRoundAndOpenNext to launchOpenedRound
    bool pre = false, blind = false, splitCur = false, tooLargeCur = false;
    int32_t splitFitCur = 0;
    uint8_t* early = nullptr;  // the block of a build that stops after round 0, begun before the device has finished
    bool earlyCopied = false;  // ... its coefficients are in it
    double tSync = 0, tWeights = 0;

    FrontierBuild(hpsdf_ctx* ctx, FrontierWorkspace* ws, const hpsdf_config* cfgIn, const hpsdf_field* field, uint64_t K, void** block, size_t* size,
                  hpsdf_build_stats* stats, int rank, int world, hpsdf_allgather_fn gather, void* gatherUser, bool trace, double t0)
        : ctx(ctx), ws(ws), cfg(configWithZeroedPads(cfgIn)), field(field), block(block), size(size), stats(stats), rank(rank), world(world),
          gather(gather), gatherUser(gatherUser), trace(trace), t0(t0), s(ctx->stream), Kj((uint32_t)(K ? K : HPSDF_DEFAULT_JOBS_PER_ROUND)),
          weighted(cfg.weighting_type != 0), replica(weighted && world > 1), mesh(innermost(field)->kind == kHostMesh),
          splitMode(ctx->fitMode == HPSDF_FIT_SPLIT && !weighted), stride0(kFrJobs * HPSDF_JOB_HEADER_DOUBLES + kFrStatusPad),
          strideK(Kj * HPSDF_JOB_HEADER_DOUBLES + kFrStatusPad), fitLds(fitLdsTable(weighted)), d(ws->d), T(ws->tmpl), hh(ws->hostHdr) {}
    FrontierBuild(const FrontierBuild&) = delete;
    ~FrontierBuild() { ctx->freeBlock(early); }

    int run();
    int leaveAfterFailure(int rc);

    // the steps of run(), in its order
    int planRound0();
    int runRound0();
    int closeRoundAndOpenNext();
    void copyEarlyBlockWhileDeviceWorks();
    int checkClosedRound();
    int finishAfterRound0();
    int selectOnGrid();
    int launchOpenedRound();
    int storeBlock();
    // what the steps share
    int exchange(void* dBuf, size_t bytesPerRank, const char* what);
    int applyWeights(const FitBlock* blocks, uint32_t maxBlocks, size_t lds, const FitTask* tasks, const uint32_t* dCount, bool round0, uint32_t base, uint32_t nMine);
    int prepareNext(uint32_t knownNodes, uint64_t knownArena, uint32_t knownMaxDeg, int roundsDone);
    int launchRoundFits(uint32_t knownMaxDeg, bool splitRound);
    int waitForRound(uint32_t want);
    void rearmForNextBuild(bool wentOn);
    FrDev initDev() const {  // what fr_init_kernel sees: the arrays as they are now, round 0's stride (where this rank's status for round 0's exchange lies)
        FrDev di = d;
        di.errStride = stride0;
        return di;
    }
    bool injectedFailure(int round) const {
        return injected && world > 1 && std::atoi(injected) == rank && std::strchr(injected, ':') && std::atoi(std::strchr(injected, ':') + 1) == round;
    }
};

int FrontierBuild::run() {
    // what every launch of this build is told (FrDev)
    d.K = Kj;
    d.rank = rank, d.world = world;
    d.weighted = weighted ? 1 : 0;
    d.replica = replica ? 1 : 0;
    d.fastFit = (ctx->fitMode == HPSDF_FIT_FAST && field->kind != kHostTreeCsg && !weighted) ? 1 : 0;
    d.splitFit = 0;
    d.errStride = stride0, d.errStrideNext = strideK;
    if (replica) {  // round 0's part of the arena, before anything can fail (PendingExchange)
        uint32_t ends[9];
        round0SliceEnds(T.nLeaves, world, ends);
        pending.rowsAt(0, (size_t)round0PartRows(ends, world) * sizeof(double));
    }
    int rc;
    if (world > 1) pending.round0Begins(stride0);
    if ((rc = makeFieldDev(ctx, field, nullptr, &fd))) return rc;
    if (injectedFailure(0)) return fail(HPSDF_ERR_OUT_OF_MEMORY, kInjectedFailureMsg);
    for (int a = 0; a < 3; ++a) {
        rm.bounds[a] = (double)(cfg.root_max[a] - cfg.root_min[a]);          // Octree.cpp:324
        rm.centre[a] = (double)((cfg.root_min[a] + cfg.root_max[a]) / 2.0f);  // Octree.cpp:322
    }
    if ((rc = planRound0())) return rc;
    if (const char* e = std::getenv("HPSDF_FRONTIER_INLINE_NODES")) inlineNodes = (uint32_t)std::strtoul(e, nullptr, 10);  // tests: 0 sends every round through the grid selection
    d.buildStamp = ++ws->buildStamp ? ws->buildStamp : ++ws->buildStamp;  // (never 0)
    d.stamps = trace ? 1u : 0u;
    ws->hostHdr->round = 0, ws->hostHdr->done = 0;  // (the mirror still shows the previous build's last round: the waits below watch it)
    if ((rc = runRound0())) return rc;
    knownNodes = T.nNodes, knownMaxDeg = 2, knownArena = T0.arenaRows;
    for (;;) {
        if ((rc = closeRoundAndOpenNext())) return rc;
        if (rounds == 0 && world == 1) copyEarlyBlockWhileDeviceWorks();
        if ((rc = waitForRound((uint32_t)rounds + 1u))) return rc;
        ++rounds;
        if ((rc = checkClosedRound())) return rc;
        if (rounds == 1 && world == 1 && hh->done && early && hh->nCoeffs == T.arenaRows && hh->nNodes == T.nNodes) return finishAfterRound0();
        ctx->freeBlock(early);
        early = nullptr;
        if (hh->done) break;
        // (as builderSelect: a total that is NaN or infinite never falls below the threshold -- the field is not finite somewhere)
        if (!(std::fabs(hh->total) <= DBL_MAX))
            return fail(HPSDF_ERR_INVALID_ARGUMENT, "the field is not a finite number at some sample point (the build's total error is NaN or infinite)");
        knownNodes = hh->nNodes, knownMaxDeg = hh->maxDegree, knownArena = hh->arenaUsed;
        if (world > 1) pending.afterHeaderRead();
        // (replica: the round's rows are exchanged too -- from here on a rank that fails enters that exchange as well.  With the grid
        // selection the part is known only when the batch kernel has run: selectOnGrid)
        if (replica && pre) pending.rowsAt(hh->roundBase, (size_t)hh->partStride * sizeof(double));
        if (!pre && (rc = selectOnGrid())) return rc;
        if ((rc = launchOpenedRound())) return rc;
    }
    return storeBlock();
}

// in place: rank r's part at r * bytesPerRank
int FrontierBuild::exchange(void* dBuf, size_t bytesPerRank, const char* what) {
    if (world == 1) return HPSDF_OK;
    const int grc = gather(gatherUser, dBuf, bytesPerRank, (void*)s);
    if (grc != 0) return fail(HPSDF_ERR_STATE, std::string("the all-gather callback failed (") + what + ")");
    return HPSDF_OK;
}

// Round 0 is every cell of the uniformly refined tree, straight from the template: this rank's share of it, and the cached upload
// of the share's lists.
int FrontierBuild::planRound0() {
    T0 = T;
    r0Tasks = ws->tmplTasks;
    r0Blocks = ws->tmplBlocks;
    r0JobP = ws->tmplJobP;
    r0Lds = ws->tmplLds;
    round0SliceEnds(T.nLeaves, world, T0.sliceFirst);
    if (world > 1) {
        const uint32_t first = T0.sliceFirst[rank], count = T0.sliceFirst[rank + 1] - first;
        int g = 1, pl = 1;
        frShape(2, false, std::max(1u, count), &g, &pl);
        const uint32_t nBl = (count + (uint32_t)g - 1u) / (uint32_t)g;
        // (replica: rank r's cells at r x part0 -- equal parts for the in-place all-gather -- and every cell's place known everywhere)
        part0 = round0PartRows(T0.sliceFirst, world);
        // this rank's task list, workgroup list and job -> arena map of round 0 depend on (rank, world, error stride, replica) alone:
        // built and uploaded once, kept on the device for the Creates that follow (no upload, no wait per Create)
        if (ws->r0Rank != rank || ws->r0World != world || ws->r0ErrStride != ws->d.errStride || ws->r0Replica != replica) {
            std::vector<FitTask>& tk = ws->hostR0Tasks;
            tk.assign(ws->hostTmplTasks.begin() + first, ws->hostTmplTasks.begin() + first + count);
            std::vector<uint64_t> jobP(T.nLeaves, ~0ull & kOffMask);
            for (uint32_t q = 0; q < count; ++q) {
                tk[q].outOff = (replica ? (uint64_t)rank * part0 : 0ull) + (uint64_t)q * frCoef(2);
                tk[q].sampleOff = (uint64_t)q * 729;
                tk[q].errSlot = (uint32_t)rank * ws->d.errStride + q * HPSDF_JOB_HEADER_DOUBLES;
                jobP[first + q] = tk[q].outOff;
            }
            if (replica)
                for (int r = 0; r < world; ++r)
                    for (uint32_t j = T0.sliceFirst[r]; j < T0.sliceFirst[r + 1]; ++j) jobP[j] = (uint64_t)r * part0 + (uint64_t)(j - T0.sliceFirst[r]) * frCoef(2);
            std::vector<FitBlock> bl(nBl);
            for (uint32_t k = 0; k < bl.size(); ++k) {
                FitBlock& fb = bl[k];
                std::memset(&fb, 0, sizeof fb);
                fb.firstTask = k * (uint32_t)g;
                fb.nTasks = (uint16_t)std::min<uint32_t>((uint32_t)g, count - k * (uint32_t)g);
                fb.degree = 2;
                fb.planesPerChunk = (uint8_t)pl;
                fb.rowStart = 0, fb.rowEnd = (uint16_t)frCoef(2);
                fb.depth = ws->hostTmplTasks[0].depth;
            }
            ws->r0Rank = ws->r0World = -1;
            HPSDF_HIP(hipMemcpyAsync(ws->r0Tasks, tk.data(), count * sizeof(FitTask), hipMemcpyHostToDevice, s));
            HPSDF_HIP(hipMemcpyAsync(ws->r0Blocks, bl.data(), bl.size() * sizeof(FitBlock), hipMemcpyHostToDevice, s));
            HPSDF_HIP(hipMemcpyAsync(ws->r0JobP, jobP.data(), jobP.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            HPSDF_HIP(hipStreamSynchronize(s));  // (pageable sources)
            ws->r0Rank = rank, ws->r0World = world, ws->r0ErrStride = ws->d.errStride, ws->r0Replica = replica;
        }
        r0Tasks = ws->r0Tasks, r0Blocks = ws->r0Blocks, r0JobP = ws->r0JobP;
        r0Lds = frLds(2, g, pl);
        T0.nTasks = count, T0.nBlocks = nBl;
        T0.arenaRows = replica ? (uint64_t)world * part0 : (uint64_t)count * frCoef(2), T0.samples = (uint64_t)count * 729;
    }
    return HPSDF_OK;
}

// fr_round_kernel closes round r and opens round r + 1 in one launch, so what round r + 1 can need -- nodes for round r's
// splits, arena rows and sample slots for round r + 1's fits -- is bounded from what the host knows when it launches it: the tree
// after round r - 1 (whose largest degree can have risen by one since).  Also decides whether round r + 1's from-scratch fits
// are split (ctx->fitMode): they are unless the sample buffer they hand their field values over in cannot be had.
int FrontierBuild::prepareNext(uint32_t knownNodes, uint64_t knownArena, uint32_t knownMaxDeg, int roundsDone) {
    const int degBound = (int)std::min<uint32_t>(knownMaxDeg + 1u, kMaxDegree);
    const uint64_t needNodes = (uint64_t)knownNodes + 8ull * Kj;
    const uint64_t needArena = knownArena + (replica ? (uint64_t)world * ((uint64_t)Kj * rowsPerJob(degBound) + 16) : (uint64_t)Kj * rowsPerJob(degBound));
    {   // hpsdf_ctx_set_build_limits: the round about to open against the context's bounds -- before anything is allocated for it, so
        // that a runaway build ends here with its statistics in the message instead of minutes later in a failed hipMalloc
        // (a mesh build cannot do without its sample buffer; the hand-over buffer of split fits -- at most 2^31 samples, 16 GiB, whatever
        // the tree's size -- is not part of what grows without bound and is not counted: counting it would make the two schedulers'
        // split decisions depend on the limit, and they promise the same bytes)
        const uint64_t needSamples = mesh ? std::min<uint64_t>((uint64_t)Kj * samplesPerJob(degBound), 1ull << 31) : 0ull;
        const uint64_t bytes = needNodes * FrontierWorkspace::kBytesPerNode + (needArena + needSamples) * sizeof(double);
        const uint64_t held = (uint64_t)ws->nodeCap * FrontierWorkspace::kBytesPerNode + (ws->arenaCap + ws->sampleCap) * sizeof(double);
        const uint64_t growBytes = needNodes * FrontierWorkspace::kBytesPerNode + needArena * sizeof(double);  // (the default limit's subject)
        const int lrc = checkBuildLimits(ctx, knownNodes, bytes, growBytes, held, &measuredLimit, (uint64_t)roundsDone, roundsDone ? hh->total : 8.0 * 8.0 * 8.0 * 8.0 * HPSDF_INITIAL_NODE_ERR,
                                         cfg.target_error_threshold);
        if (lrc) return lrc;
    }
    if (needNodes > 0xFFFFFFF0ull) return fail(HPSDF_ERR_BUILD_LIMIT, "build limit: the device-side frontier indexes nodes with 32 bits");
    hipError_t e = ws->ensureNodes((uint32_t)needNodes, s);
    if (e == hipSuccess) e = ws->ensureArena(needArena, knownArena, s);
    if (e != hipSuccess) return hipFail(e, "frontier buffers");
    splitOpen = splitMode && degBound >= ctx->splitMinDegree;
    samplesTooLarge = false;
    if (mesh || splitOpen) {
        // (the round's own count decides on the device whether it splits -- the host scheduler's rule, FrHdr::splitRound; the host
        // provides for what the round can need, up to the 2^31 samples a split round may have)
        uint64_t need = (uint64_t)Kj * samplesPerJob(degBound);
        if (need > (1ull << 31)) {
            if (mesh) samplesTooLarge = true;  // (a mesh build fails when that round comes)
            need = 1ull << 31;
        }
        if (!samplesTooLarge && (e = ws->ensureSamples(need, s)) != hipSuccess) {
            if (mesh) return hipFail(e, "frontier sample buffer");
            (void)hipGetLastError();  // no room for the hand-over buffer: the exact fit needs none
            splitOpen = false;
        }
    }
    d.sampleCap = ws->sampleCap;
    return HPSDF_OK;
}

// Weighted builds, once per round behind the fits: |mean FApprox| of every fit (fit_weight_kernel, straight into pinned
// host memory) -> the weight, with the HOST's pow / exp (Octree.cpp:1224-1226, :1246: the libm the oracle and the host
// scheduler call; a device pow would have to match it bit for bit) -> error * weight on the device (:1078-1086).
// Everything else of the round -- selection, tasks, decision, bookkeeping, packing -- stays where it is.
// (base, nMine: this rank's run of error slots and its jobs of the round)
int FrontierBuild::applyWeights(const FitBlock* blocks, uint32_t maxBlocks, size_t lds, const FitTask* tasks, const uint32_t* dCount, bool round0, uint32_t base,
                                uint32_t nMine) {
    HPSDF_HIP(launchFitWeight(s, blocks, maxBlocks, lds, tasks, ws->arena, d.means, ctx->dTables, dCount));
    const uint32_t stamp = ++ws->flagStamp;
    FR_LAUNCH(fr_means_done_kernel, frLaunchMeansDone, s, d, stamp);
    const double ts = frNow();
    {
        const volatile uint32_t* flag = ws->hostFlag;
        if (!watchWord(&flag[1], stamp, 2.0e3)) HPSDF_HIP(hipStreamSynchronize(s));
        std::atomic_thread_fence(std::memory_order_acquire);
        if (flag[1] != stamp) return fail(HPSDF_ERR_STATE, "frontier: the round's means did not arrive");
    }
    const double tw = frNow();
    tSync += tw - ts;
    const uint32_t nJobs = world == 1 ? std::min<uint32_t>(ws->hostFlag[0], kFrJobs) : std::min<uint32_t>(nMine, kFrJobs);
    const double* mean = ws->hostMeans + base;
    double* w = ws->hostWeights + base;
    const uint32_t step = round0 ? 9u : 1u;  // round 0: every job is a coarse cell with one fit (slot 0 of its nine)
    for (uint32_t i = 0; i < nJobs * 9u; i += step) w[i] = nearnessWeight(cfg, mean[i]);
    std::atomic_thread_fence(std::memory_order_release);
    tWeights += frNow() - tw;
    FR_LAUNCH(fr_weigh_kernel, frLaunchWeigh, s, d, round0 ? 1u : 9u, base, nJobs);
    return HPSDF_OK;
}

// a round's fits, from the lists the device wrote (fit_mesh.hip, fit.hip; grids are upper bounds)
int FrontierBuild::launchRoundFits(uint32_t knownMaxDeg, bool splitRound) {
    const int degHi = (int)std::min<uint32_t>(kMaxDegree - 1, knownMaxDeg + 1);
    const uint32_t taskBound = 9u * Kj;
    bool degHiDone = false;
    FieldDev fdr = fd;
    if (mesh) {
        for (int deg = 2; deg <= degHi; ++deg)
            HPSDF_HIP(launchMeshSampleRange(s, d.tasks, &d.hdr->degTasks[deg][0], std::min<uint32_t>(taskBound, 65535u), deg, ctx->dTables, fd,
                                            rm, ws->samples));
        fdr.kind = kFieldSamples;
        fdr.samples = ws->samples;
    } else if (splitRound) {
        fdr.samples = ws->samples;  // (the exact kernel writes the field values of split fits there)
    }
    // One launch for every degree of the round (fit_kernels.hpp fit_multi_kernel); the matrix-core fit and
    // HPSDF_FRONTIER_SPLIT_FITS=1 keep one launch per degree, side by side on three streams.
    static const bool splitFits = std::getenv("HPSDF_FRONTIER_SPLIT_FITS") != nullptr;
    if (!d.fastFit && !splitFits) {
        size_t lds = 0;
        for (int deg = 2; deg <= degHi; ++deg) lds = std::max(lds, fitLds[deg]);
        HPSDF_HIP(launchFitMulti(s, d.blocks, taskBound, lds, d.tasks, ws->arena, d.errs, ctx->dTables, fdr, rm, &d.hdr->nBlocks));
        degHiDone = true;
    }
    const bool fork = !degHiDone && degHi > 2 && std::getenv("HPSDF_FRONTIER_ONE_STREAM") == nullptr;
    if (fork) HPSDF_HIP(hipEventRecord(ws->forkEv, s));
    bool used[FrontierWorkspace::kSide] = {false, false, false};
    for (int deg = 2; deg <= degHi && !degHiDone; ++deg) {
        hipStream_t fs = s;
        if (fork && deg > 2) {
            const int k = (deg - 3) % FrontierWorkspace::kSide;
            fs = ws->side[k];
            if (!used[k]) HPSDF_HIP(hipStreamWaitEvent(fs, ws->forkEv, 0));
            used[k] = true;
        }
        if (d.fastFit && deg >= 4 && deg <= 11)
            HPSDF_HIP(launchFitMfma(fs, deg, d.blocks, taskBound, d.tasks, ws->arena, d.errs, ctx->dTables, fdr, rm, &d.hdr->degBlocks[deg][0]));
        else
            HPSDF_HIP(launchFit(fs, deg <= 8 ? deg : 0, 1, d.blocks, taskBound, fitLds[deg], d.tasks, ws->arena, d.errs, nullptr,
                                ctx->dTables, fdr, rm, &d.hdr->degBlocks[deg][0]));
    }
    for (int k = 0; k < FrontierWorkspace::kSide; ++k)
        if (used[k]) {
            HPSDF_HIP(hipEventRecord(ws->joinEv[k], ws->side[k]));
            HPSDF_HIP(hipStreamWaitEvent(s, ws->joinEv[k], 0));
        }
    if (splitRound)  // the rows below the top degree of the split fits, from the samples the exact kernel left (H children: degree <= knownMaxDeg)
        for (int deg = std::max(2, ctx->splitMinDegree); deg <= (int)std::min<uint32_t>(knownMaxDeg, 11u); ++deg)
            HPSDF_HIP(launchFitMfmaLow(s, deg, d.tasks, &d.hdr->lowTasks[deg][0], 0u, 0u, 8u * Kj, ws->arena, ctx->dTables, ws->samples, rm, fd.leftAssoc));
    if (weighted) {
        size_t lds = 0;
        for (int deg = 2; deg <= degHi; ++deg) lds = std::max(lds, fitLds[deg]);
        int rcw;
        const uint32_t mine = world == 1 ? 0u : hh->sliceFirst[rank + 1] - hh->sliceFirst[rank];  // (one rank: the device says how many)
        if ((rcw = applyWeights(d.blocks, taskBound, lds, d.tasks, &d.hdr->nBlocks, false, world == 1 ? 0u : (uint32_t)rank * strideK, mine))) return rcw;
    }
    return HPSDF_OK;
}

// The round is over for the host when the header's mirror shows the next round number: the closing workgroup writes it into
// pinned memory behind a system-scope fence.
int FrontierBuild::waitForRound(uint32_t want) {
    const double ts = frNow();
    const volatile uint32_t* roundWord = &hh->round;
    if (!watchWord(roundWord, want, 2.0e3)) {  // two milliseconds of watching, then the ordinary wait
        HPSDF_HIP(hipStreamSynchronize(s));
        if (*roundWord != want) {
            // The stream is idle and the mirror still shows the old round: the pinned mirror is not coherent on this system.
            // Fetch the header itself and let it decide.
            HPSDF_HIP(hipMemcpy(ws->hostHdr, d.hdr, kFrHdrCopyBytes, hipMemcpyDeviceToHost));
            if (hh->round != want) return fail(HPSDF_ERR_STATE, "frontier: a round ended without advancing");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    tSync += frNow() - ts;
    return HPSDF_OK;
}

// the launch that leaves the workspace ready for this context's next build (FrontierWorkspace::clean)
void FrontierBuild::rearmForNextBuild(bool wentOn) {
    ws->clean = frLaunchInit(s, initDev(), T0) == hipSuccess, ws->cleanRank = rank, ws->cleanWorld = world;
    ws->lastWentOn = wentOn;
}

int FrontierBuild::runRound0() {
    int rc;
    hipError_t e = ws->ensureArena(std::max<uint64_t>(1, T0.arenaRows), 0, s);
    if (e == hipSuccess && mesh) e = ws->ensureSamples(std::max<uint64_t>(1, T0.samples), s);
    if (e != hipSuccess) return hipFail(e, "frontier buffers");
    if ((rc = prepareNext(T.nNodes, T0.arenaRows, 2u, 0))) return rc;
    d.target = cfg.target_error_threshold;
    if (!ws->clean || ws->cleanRank != rank || ws->cleanWorld != world) FR_LAUNCH(fr_init_kernel, frLaunchInit, s, initDev(), T0);
    ws->clean = false;
    FieldDev fdr = fd;
    if (mesh) {
        HPSDF_HIP(launchMeshSample(s, r0Tasks, T0.nTasks, 2, ctx->dTables, fd, rm, ws->samples));
        fdr.kind = kFieldSamples;
        fdr.samples = ws->samples;
    }
    // (one rank: the rows also go straight into pinned host memory -- if the build stops after this round they are its packed store)
    HPSDF_HIP(launchFit(s, 2, 1, r0Blocks, T0.nBlocks, r0Lds, r0Tasks, ws->arena, d.errs, world == 1 ? ws->pinnedDev : nullptr, ctx->dTables, fdr, rm));
    if (weighted && (rc = applyWeights(r0Blocks, T0.nBlocks, r0Lds, r0Tasks, nullptr, true, world == 1 ? 0u : (uint32_t)rank * stride0,
                                       T0.sliceFirst[rank + 1] - T0.sliceFirst[rank])))
        return rc;
    if (replica) {
        if (pending.rowsBytes != (size_t)part0 * sizeof(double)) return fail(HPSDF_ERR_STATE, "frontier: round 0's part of the arena");
        pending.rowsEntered();
        if ((rc = exchange(ws->arena, pending.rowsBytes, "round 0's rows"))) return rc;
    }
    if ((rc = exchange(d.errs, (size_t)stride0 * sizeof(double), "round 0"))) return rc;
    pending.afterRound0Exchanges(strideK);
    d.errStride = strideK;  // (of the exchange that comes next: where a failing rank leaves its status)
    return HPSDF_OK;
}

// close round `rounds`, open the next
int FrontierBuild::closeRoundAndOpenNext() {
    int rc;
    pre = (uint64_t)knownNodes + 8ull * Kj <= inlineNodes;
    splitCur = splitOpen, tooLargeCur = samplesTooLarge;
    FrDev dk = d;
    dk.splitFit = splitFitCur = splitCur ? std::max(2, ctx->splitMinDegree) : 0;
    if (rounds == 0) {
        dk.batchIdx = ws->tmplLeaves, dk.batchErr = ws->tmplErr, dk.jobP = r0JobP, dk.jobH = r0JobP;
        dk.errStride = stride0;
    }
    FR_LAUNCH(fr_round_kernel, frLaunchRound, s, dk, rounds == 0 ? T.nLeaves : Kj, (pre ? 1 : 0) | (ws->lastWentOn && pre ? 2 : 0));
    // From the second round on the fits are launched without waiting for the header (one rank, no host step in between): what they
    // need to know is on the device -- their lists and counts -- and a build that has stopped leaves them nothing to do.  The
    // largest degree may have risen once more than the host knows.
    const bool noBlind = std::getenv("HPSDF_FRONTIER_NO_BLIND") != nullptr;  // (tests, comparisons)
    // Behind round 0 too when this context's last build went on past it (the guess that also hands round 0's total to the last
    // workgroup): the second round's fits then start when the closing launch ends instead of a host round trip later (~15 us); a
    // build that does stop there leaves two empty launches behind.
    blind = (rounds >= 1 || ws->lastWentOn) && pre && world == 1 && !weighted && !frSyncEveryLaunch() && !noBlind;
    if (blind) {
        if (mesh && tooLargeCur) return fail(HPSDF_ERR_UNSUPPORTED, "round too large for the sampled mesh path");
        d.splitFit = splitFitCur;
        FrDev de = d;  // (not dk: round 0's closing launch reads the template's batch, the lists are written for the next one)
        FR_LAUNCH(fr_emit_kernel, frLaunchEmit, s, de, Kj);
        if ((rc = launchRoundFits(std::min<uint32_t>(knownMaxDeg + 1u, kMaxDegree), splitCur))) return rc;
    }
    return HPSDF_OK;
}

// One rank, round 0: a build that stops here has its packed store in pinned memory already (the fit wrote it there too), and
// everything else of its block is known in advance: write that part while the device works
void FrontierBuild::copyEarlyBlockWhileDeviceWorks() {
    const uint64_t nc0 = T.arenaRows, nn0 = T.nNodes;
    early = (uint8_t*)ctx->allocBlock(blockBytes(nc0, nn0));
    if (!early) return;
    std::memcpy(early, &nc0, 8);
    std::memcpy(early + blockNodeCountAt(nc0), &nn0, 8);
    std::memcpy(early + blockNodesAt(nc0), ws->hostNodesAfterRound0.data(), sizeof(hpsdf_node) * (size_t)nn0);
    std::memcpy(early + blockConfigAt(nc0, nn0), &cfg, sizeof cfg);
    // ... and the rows themselves as soon as the closing launch says that the fit before it has finished -- long before it
    // can say whether the build stops here (the running total is 4096 dependent additions away): 320 KB out of memory the
    // GPU has just written take a core ~20 us, which now pass while the device works.  In pieces, with an eye on the round
    // word: a build that goes on must not wait for a copy it will not use.  (Two words under one limit: not watchWord.)
    const volatile uint32_t* landed = &hh->landed;
    const volatile uint32_t* roundWord = &hh->round;
    const double limit = frNow() + 2.0e3;
    while (*landed != d.buildStamp && *roundWord == 0 && frNow() < limit) frCpuRelax();
    if (*landed == d.buildStamp) {
        std::atomic_thread_fence(std::memory_order_acquire);
        const size_t total = 8 * (size_t)nc0, piece = 32768;
        size_t at = 0;
        for (; at < total && (*roundWord == 0 || *(const volatile uint32_t*)&hh->done); at += piece) std::memcpy(early + kBlockCoeffsAt + at, ws->pinned + at, std::min(piece, total - at));
        earlyCopied = at >= total;
    }
}

// what the header says about the round that has just closed
int FrontierBuild::checkClosedRound() {
    if (world > 1 && hh->rPad)
        return fail(HPSDF_ERR_STATE, "rank " + std::to_string(hh->rPad - 1) + " failed in round " + std::to_string(rounds - 1) + ": its own error was returned there");
    if (hh->overflow & 1u) return fail(HPSDF_ERR_STATE, "frontier: node capacity exceeded");
    if (hh->overflow & 4u) return fail(HPSDF_ERR_STATE, "frontier: a workgroup of the round's kernel did not arrive");
    if (trace) {
        std::fprintf(stderr, "[frontier round %d] lead (cycles): wait-all %lld close %lld", rounds - 1, (long long)(hh->dbg[10] - hh->dbg[9]),
                     (long long)(hh->dbg[11] - hh->dbg[10]));
        if (!hh->done && pre) {
            std::fprintf(stderr, " | select %lld batch", (long long)(hh->dbg[0] - hh->dbg[11]));
            for (int k = 1; k <= 8; ++k) std::fprintf(stderr, " %lld", (long long)(hh->dbg[k] - hh->dbg[k - 1]));
            std::fprintf(stderr, " | total+commit %lld", (long long)(hh->dbg[12] - hh->dbg[8]));
        }
        std::fprintf(stderr, " | chain %lld (first operands %lld, first 2048 additions %lld)", (long long)(hh->dbg[14] - hh->dbg[13]), (long long)(hh->dbg[15] - hh->dbg[13]),
                     (long long)(hh->dbg[16] - hh->dbg[15]));
        std::fprintf(stderr, "\n");
    }
    return HPSDF_OK;
}

// the build stopped after round 0 and the block begun early is its block
int FrontierBuild::finishAfterRound0() {
    if (!earlyCopied) std::memcpy(early + kBlockCoeffsAt, ws->pinned, 8 * (size_t)T.arenaRows);
    rearmForNextBuild(false);
    *block = early;
    *size = blockBytes(T.arenaRows, T.nNodes);
    early = nullptr;
    if (stats) fillStats(hh, hh->nNodes, hh->nCoeffs, ctx->fitMode, stats);
    if (trace) std::fprintf(stderr, "[frontierCreate] us: total %.0f (waiting for the device %.0f, stopped after round 0)\n", frNow() - t0, tSync);
    return HPSDF_OK;
}

// a large tree: the selection as a grid, then batch and lists (the header's arenaUsed lags one round: launchOpenedRound bounds it)
int FrontierBuild::selectOnGrid() {
    FrDev dl = d;
    dl.splitFit = splitFitCur;
    FR_LAUNCH(fr_select_kernel, frLaunchSelect, s, dl, knownNodes);
    FR_LAUNCH(fr_batch_kernel, frLaunchBatch, s, dl);
    FR_LAUNCH(fr_tasks_kernel, frLaunchTasks, s, dl, Kj);
    if (replica) {
        // Where the round's part of the arena lies is the batch kernel's decision, and the exchange below needs it.  The
        // context's stream does not synchronise with the null stream (hipStreamNonBlocking): a plain hipMemcpy right behind the
        // launches would fetch the PREVIOUS round's roundBase / partStride.  Wait for the three kernels, then fetch.
        HPSDF_HIP(hipStreamSynchronize(s));
        HPSDF_HIP(hipMemcpy(ws->hostHdr, d.hdr, kFrHdrCopyBytes, hipMemcpyDeviceToHost));
        pending.rowsAt(hh->roundBase, (size_t)hh->partStride * sizeof(double));
    }
    return HPSDF_OK;
}

// The fits of the round that the closing launch opened, and their exchanges.
// (A rank whose share fails from here on knows which exchanges the others are heading for, and how large their parts are: with
// the grid selection that is only true once the batch kernel has spoken, hence the order.  A failed launch of the three
// selection kernels themselves -- a lost device, not a full one -- is not covered: that rank enters the errors' exchange alone.)
int FrontierBuild::launchOpenedRound() {
    int rc;
    if (injectedFailure(rounds)) return fail(HPSDF_ERR_OUT_OF_MEMORY, kInjectedFailureMsg);
    if (mesh && tooLargeCur) return fail(HPSDF_ERR_UNSUPPORTED, "round too large for the sampled mesh path");
    if (pre && !blind) {
        FrDev de = d;
        de.splitFit = splitFitCur;
        FR_LAUNCH(fr_emit_kernel, frLaunchEmit, s, de, Kj);
    }
    // capacities of the launch that closes this round; the arena may move: nothing that writes it is in flight
    if ((rc = prepareNext(knownNodes, knownArena + (pre ? 0ull : (uint64_t)(replica ? world : 1) * ((uint64_t)Kj * rowsPerJob((int)knownMaxDeg) + 16)), knownMaxDeg, rounds))) return rc;
    d.splitFit = splitFitCur;
    if (!blind && (rc = launchRoundFits(knownMaxDeg, splitCur))) return rc;
    if (replica) {
        pending.rowsEntered();
        if ((rc = exchange(ws->arena + pending.rowsOff, pending.rowsBytes, "a round's rows"))) return rc;  // (the arena may have moved: offset, not pointer)
    }
    if (frSyncEveryLaunch()) std::fprintf(stderr, "[frontier] fits of round %d ... %s\n", rounds, hipGetErrorString(hipStreamSynchronize(s)));
    if ((rc = exchange(d.errs, (size_t)strideK * sizeof(double), "a round's errors"))) return rc;
    pending.errorsExchanged();
    return HPSDF_OK;
}

// ReallocCoeffs, and Octree::ToMemoryBlock (Octree.cpp:424-456: [u64 nCoeffs][f64 x nCoeffs][u64 nNodes][Node x nNodes][Config]): the
// device writes coefficients and node array into pinned host memory (fr_store_kernel), the host moves each part into the block
// when the mirror says it is there -- the node array while the coefficients are still landing
int FrontierBuild::storeBlock() {
    int rc;
    const uint64_t nc = hh->nCoeffs, nn = hh->nNodes;
    {
        hipError_t e = ws->ensurePinned(8 * (size_t)nc + sizeof(hpsdf_node) * (size_t)nn);
        if (e != hipSuccess) return hipFail(e, "block staging");
        d.store = ws->pinnedDev;
        FR_LAUNCH(fr_subtree_kernel, frLaunchSubtree, s, d, (uint32_t)nn);
        if (world > 1 && !replica) {
            // the packed store from one all-gather of the ranks' pack buffers (each rank's own segments in node order)
            FR_LAUNCH(fr_packpos_kernel, frLaunchPackPos, s, d);
            HPSDF_HIP(hipStreamSynchronize(s));
            uint64_t stride = 1;
            for (int r = 0; r < world; ++r) stride = std::max<uint64_t>(stride, hh->packCount[r]);
            stride = (stride + 15) & ~15ull;
            e = ws->ensurePack((uint64_t)world * stride, s);
            if (e != hipSuccess) return hipFail(e, "pack buffers");
            d.packStride = stride;
            FR_LAUNCH(fr_pack_kernel, frLaunchPack, s, d, knownNodes);
            if ((rc = exchange(d.pack, (size_t)stride * sizeof(double), "the packed coefficients"))) return rc;
        }
        FR_LAUNCH(fr_store_kernel, frLaunchStore, s, d, (uint32_t)nn);
    }
    const size_t bytes = blockBytes(nc, nn);
    uint8_t* p = (uint8_t*)ctx->allocBlock(bytes);
    if (!p) {
        (void)hipStreamSynchronize(s);
        return fail(HPSDF_ERR_OUT_OF_MEMORY, "malloc of the memory block failed");
    }
    const double tc = frNow();
    std::memcpy(p, &nc, 8);
    std::memcpy(p + blockNodeCountAt(nc), &nn, 8);
    std::memcpy(p + blockConfigAt(nc, nn), &cfg, sizeof cfg);
    for (int part = 0; part < 2; ++part) {  // 0: the node array, 1: the coefficients
        if (!watchWord(&hh->stored[part], d.buildStamp, 2.0e3)) {  // (two milliseconds of watching, then the ordinary wait: the launch has finished, its stores are there)
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                ctx->freeBlock(p);
                return hipFail(e, "block download");
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (part == 0)
            std::memcpy(p + blockNodesAt(nc), ws->pinned + 8 * (size_t)nc, sizeof(hpsdf_node) * (size_t)nn);
        else
            std::memcpy(p + kBlockCoeffsAt, ws->pinned, 8 * (size_t)nc);
    }
    const double tcopy = frNow() - tc;
    *block = p;
    *size = bytes;
    if (stats) fillStats(hh, nn, nc, ctx->fitMode, stats);
    rearmForNextBuild(rounds > 1);
    if (trace)
        std::fprintf(stderr, "[frontierCreate] us: total %.0f (waiting for the device %.0f over %d rounds, weights on the host %.0f, block download %.0f)\n",
                     frNow() - t0, tSync, rounds, tWeights, tcopy);
    return HPSDF_OK;
}

// A build that failed.  Several ranks, with an exchange pending: this rank still enters it, then returns its own error text.
int FrontierBuild::leaveAfterFailure(int rcBody) {
    if (world > 1 && pending.errors != PendingExchange::kNone) {
        const std::string own = hpsdf_last_error();
        const size_t stride = pending.errStride;
        const unsigned long long ones = ~0ull;
        if (pending.rows) (void)gather(gatherUser, ws->arena + pending.rowsOff, pending.rowsBytes, (void*)s);  // (replica: the others exchange the round's rows first)
        // (this rank's errors of the round were never written: zeros instead of whatever the buffer held -- the others' round kernels
        // read every job's errors before their leader looks at the status)
        if (hipMemsetAsync(ws->d.errs + (size_t)rank * stride, 0, stride * sizeof(double), s) == hipSuccess &&
            hipMemcpyAsync(ws->d.errs + (size_t)rank * stride + (stride - 1), &ones, sizeof ones, hipMemcpyHostToDevice, s) == hipSuccess)
            (void)gather(gatherUser, ws->d.errs, stride * sizeof(double), (void*)s);
        (void)hipStreamSynchronize(s);
        return fail(rcBody, own);
    }
    // A build that fails leaves nothing in flight: the round kernel's leader publishes the round number -- which is what the host
    // watches -- BEFORE it prepares the next round, so a failure noticed right there (another rank's status, an overflow) would
    // otherwise return with that kernel still writing the header's mirror and the lists, into buffers the caller may free next.
    const std::string own = hpsdf_last_error();
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    return fail(rcBody, own);
}

}  // namespace

int frontierCreate(hpsdf_ctx* ctx, const hpsdf_config* cfgIn, const hpsdf_field* field, uint64_t K, void** block, size_t* size,
                   hpsdf_build_stats* stats, int rank, int world, hpsdf_allgather_fn gather, void* gatherUser) {
    if (world < 1 || world > 8 || rank < 0 || rank >= world) return fail(HPSDF_ERR_INVALID_ARGUMENT, "bad rank/world (1..8 ranks)");
    if (world > 1 && !gather) return fail(HPSDF_ERR_INVALID_ARGUMENT, "a multi-rank build needs an all-gather");
    const bool trace = std::getenv("HPSDF_TRACE") != nullptr;
    const double t0 = frNow();
    if (const int rc = validateBuildConfig(cfgIn)) return rc;
    HPSDF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (!ctx->frontierScratch) {
        auto w = std::make_shared<FrontierWorkspace>();
        const hipError_t e = w->init(ctx->device, s);
        if (e != hipSuccess) return hipFail(e, "frontier workspace");
        ctx->frontierScratch = w;
    }
    FrontierWorkspace* ws = static_cast<FrontierWorkspace*>(ctx->frontierScratch.get());
    if (ws->inUse) return fail(HPSDF_ERR_STATE, "one Create at a time per context");
    ws->inUse = true;
    struct Release {
        FrontierWorkspace* w;
        ~Release() { w->inUse = false; }
    } release{ws};
    FrontierBuild b(ctx, ws, cfgIn, field, K, block, size, stats, rank, world, gather, gatherUser, trace, t0);
    if (b.weighted) {
        const hipError_t e = ws->ensureWeighting();
        if (e != hipSuccess) return hipFail(e, "frontier weighting buffers");
    }
    {
        const hipError_t e = ws->ensureRanks(world, s);
        if (e != hipSuccess) return hipFail(e, "frontier buffers");
    }
    const int rc = b.run();
    return rc ? b.leaveAfterFailure(rc) : rc;
}

}  // namespace hpsdf
