// C ABI of include/hpsdf.h: the stepwise build, Create (on the host scheduler, or handed to the device frontier) and the continuity entries.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "builder.hpp"
#include "continuity.hpp"
#include "frontier.hpp"
#include "runtime.hpp"

using namespace hpsdf;

static thread_local hpsdf_continuity_stats g_lastContinuity = {};

extern "C" {

// ---------------------------------------------------------------------------- build
int hpsdf_build_begin(const hpsdf_config* cfg, const hpsdf_build_opts* opts, hpsdf_build** out) {
    HPSDF_TRY
    if (!cfg || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    hpsdf_build* b = new hpsdf_build();
    int rc = builderBegin(b, cfg, opts);
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_build_destroy(hpsdf_build* b) {
    delete b;
    return HPSDF_OK;
}

int hpsdf_build_round_select(hpsdf_build* b, uint64_t* nJobs) {
    HPSDF_TRY
    if (!b || !nJobs) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderSelect(b, nJobs);
    HPSDF_CATCH
}

int hpsdf_build_round_jobs(const hpsdf_build* b, hpsdf_job* out) {
    HPSDF_TRY
    if (!b || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderJobs(b, out);
    HPSDF_CATCH
}

int hpsdf_build_round_slice(const hpsdf_build* b, int rank, uint64_t* first, uint64_t* count) {
    if (!b || rank < 0 || rank >= b->world) return fail(HPSDF_ERR_INVALID_ARGUMENT, "bad rank");
    if (!b->roundOpen) return fail(HPSDF_ERR_STATE, "no open round");
    if (first) *first = b->slices[rank].first;
    if (count) *count = b->slices[rank].count;
    return HPSDF_OK;
}

int hpsdf_build_round_max_slice(const hpsdf_build* b, uint64_t* n) {
    if (!b || !n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (!b->roundOpen) return fail(HPSDF_ERR_STATE, "no open round");
    uint64_t m = 0;
    for (const auto& s : b->slices) m = std::max(m, s.count);
    *n = m;
    return HPSDF_OK;
}

int hpsdf_build_round_compute(hpsdf_build* b, hpsdf_ctx* ctx, const hpsdf_field* field) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    return builderCompute(b, ctx, field);
    HPSDF_CATCH
}

int hpsdf_build_round_results_device(hpsdf_build* b, double** dHeaders, uint64_t* n) {
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    if (!b->roundOpen || !b->computed) return fail(HPSDF_ERR_STATE, "round not computed");
    if (b->weighted) return fail(HPSDF_ERR_UNSUPPORTED, "weighted builds apply the weight on the host: use hpsdf_build_round_results_host");
    if (dHeaders) *dHeaders = b->ws ? b->ws->errs.dev : nullptr;
    if (n) *n = b->slices[b->rank].count * HPSDF_JOB_HEADER_DOUBLES;
    return HPSDF_OK;
}

int hpsdf_build_round_results_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out) {
    HPSDF_TRY
    if (!b || !ctx || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (!b->roundOpen || !b->computed) return fail(HPSDF_ERR_STATE, "round not computed");
    const uint64_t n = b->slices[b->rank].count * HPSDF_JOB_HEADER_DOUBLES;
    HPSDF_HIP(hipSetDevice(ctx->device));
    const uint64_t nSlots = std::max<uint64_t>(1, n);
    if (n) {
        HPSDF_HIP(hipMemcpyAsync(b->ws->errs.host, b->ws->errs.dev, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (b->weighted)
            HPSDF_HIP(hipMemcpyAsync(b->ws->errs.host + nSlots, b->ws->errs.dev + nSlots, n * sizeof(double),
                                     hipMemcpyDeviceToHost, ctx->stream));
    }
    HPSDF_HIP(hipStreamSynchronize(ctx->stream));
    if (n) std::memcpy(out, b->ws->errs.host, n * sizeof(double));
    if (b->weighted) {
        // Octree.cpp:1078-1086: error * weight, the weight from |mean FApprox| (:1224-1226 / :1246)
        const double* mean = b->ws->errs.host + nSlots;
        for (uint64_t i = 0; i < n; ++i) out[i] = out[i] * nearnessWeight(b->cfg, mean[i]);
    }
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_build_round_apply(hpsdf_build* b, const double* headers) {
    HPSDF_TRY
    if (!b || !headers) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderApply(b, headers);
    HPSDF_CATCH
}

int hpsdf_build_rows_counts(const hpsdf_build* b, uint64_t* counts_per_rank) {
    HPSDF_TRY
    if (!b || !counts_per_rank) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderRowsCounts(b, counts_per_rank);
    HPSDF_CATCH
}

int hpsdf_build_rows_pack_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out) {
    HPSDF_TRY
    if (!b || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderRowsPackHost(b, ctx, out);
    HPSDF_CATCH
}

int hpsdf_build_rows_unpack_host(hpsdf_build* b, hpsdf_ctx* ctx, const double* const* parts) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    return builderRowsUnpackHost(b, ctx, parts);
    HPSDF_CATCH
}

int hpsdf_build_node_rows_host(hpsdf_build* b, hpsdf_ctx* ctx, uint64_t node_idx, double* out, uint64_t* n_rows) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    return builderNodeRowsHost(b, ctx, node_idx, out, n_rows);
    HPSDF_CATCH
}

int hpsdf_build_round_inject(hpsdf_build* b, uint64_t job, const double* pCoeffs, const double* hCoeffs) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    return builderInject(b, job, pCoeffs, hCoeffs);
    HPSDF_CATCH
}

int hpsdf_build_layout(hpsdf_build* b, uint64_t* nCoeffsTotal, uint64_t* counts) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    int rc = builderLayout(b);
    if (rc) return rc;
    if (nCoeffsTotal) *nCoeffsTotal = b->nCoeffsTotal;
    if (counts)
        for (int r = 0; r < b->world; ++r) counts[r] = b->packCounts[r];
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_build_pack_device(hpsdf_build* b, hpsdf_ctx* ctx, double** dPack, uint64_t* n) {
    HPSDF_TRY
    if (!b) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null build");
    return builderPackDevice(b, ctx, dPack, n);
    HPSDF_CATCH
}

int hpsdf_build_pack_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out) {
    HPSDF_TRY
    if (!b || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderPackHost(b, ctx, out);
    HPSDF_CATCH
}

int hpsdf_build_assemble(hpsdf_build* b, const double* const* packs, void** block, size_t* size) {
    HPSDF_TRY
    if (!b || !block || !size) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return builderAssemble(b, packs, block, size);
    HPSDF_CATCH
}

int hpsdf_build_get_stats(const hpsdf_build* b, hpsdf_build_stats* out) {
    if (!b || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *out = b->stats;
    out->total_error = b->total;
    out->n_nodes = b->nodes.size();
    return HPSDF_OK;
}

// A block that builderAssemble malloc'd, for a context with its own block allocator (hpsdf_ctx_set_block_allocator): moved there.
static int adoptBlock(hpsdf_ctx* ctx, void** block, size_t size) {
    if (!ctx->blockAlloc) return HPSDF_OK;
    void* q = ctx->allocBlock(size);
    if (!q) {
        std::free(*block);
        *block = nullptr;
        return fail(HPSDF_ERR_OUT_OF_MEMORY, "the block allocator returned no memory");
    }
    std::memcpy(q, *block, size);
    std::free(*block);
    *block = q;
    return HPSDF_OK;
}

// The tail of every Create (Octree.cpp:341-344): the continuity pass over a block that was built, when the configuration asks for it.
// Several ranks run it each on their identical copy (deterministic: no exchange).  `rc` is the build's status and comes back
// unless the pass itself fails: then the block is freed and the outputs are zeroed.
static int continuityAfterCreate(hpsdf_ctx* ctx, const hpsdf_config* cfg, void** block, size_t* size, int rc) {
    std::memset(&g_lastContinuity, 0, sizeof g_lastContinuity);
    if (rc || !cfg->continuity_enforce) return rc;
    std::string err;
    rc = continuityPostProcess(*block, *size, 0.0, 0, 0, &g_lastContinuity, err, ctx);
    if (rc) {
        setError(err);
        ctx->freeBlock(*block);
        *block = nullptr;
        *size = 0;
    }
    return rc;
}

}  // extern "C"

namespace {

// What the ranks of a host-scheduler build hand each other, through the caller's all-gather.  The scheduler keeps its results in host
// memory (the weight's pow / exp run there), so every exchange is staged through one device buffer: this rank's part up, the in-place
// all-gather, everything down.  ONE rank exchanges nothing: no staging buffer, no callback, no copy, and part(0) is the array it came with.
struct RankExchange {
    hpsdf_ctx* ctx;
    int rank, world;
    hpsdf_allgather_fn gather;
    void* user;
    struct Stage {
        double* d = nullptr;
        uint64_t cap = 0;
        ~Stage() {
            if (d) (void)hipFree(d);
        }
    } stage;
    std::vector<double> all;
    uint64_t stride = 0;  // doubles per rank in `all` after an exchange
    int exchanges = 0;
    const double* own = nullptr;  // one rank: what it entered the last exchange with

    const double* part(int r) const { return world == 1 ? own : all.data() + (uint64_t)r * stride; }

    // every rank's `mine` (count doubles, padded to `pad`) -> all[world][stride], stride = pad + 1: the last double of a rank's
    // part is its STATUS (0: fine).  A rank whose share of the round failed (localRc: device memory, a launch) still enters the
    // exchange, with its status set, and returns its own error afterwards; the others find the status, and return
    // HPSDF_ERR_STATE instead of waiting in the next collective for a rank that has left.
    int operator()(const double* mine, uint64_t count, uint64_t pad, const char* what, int localRc) {
        if (world == 1) {
            own = mine;
            return localRc;
        }
#ifdef HPSDF_TEST_HOOKS  // (lib/libhpsdf_hooks.so, built for tests/: the production library does not look at the variable)
        const char* injected = std::getenv("HPSDF_TEST_FAIL_RANK");  // "<rank>:<exchange number>"
#else
        constexpr const char* injected = nullptr;  // (the statements that look at it fold away: the production library holds no trace of the hook)
#endif
        if (injected && !localRc && std::atoi(injected) == rank && std::strchr(injected, ':') && std::atoi(std::strchr(injected, ':') + 1) == exchanges)
            localRc = fail(HPSDF_ERR_OUT_OF_MEMORY, kInjectedFailureMsg);
        ++exchanges;
        std::string ownError = localRc ? std::string(hpsdf_last_error()) : std::string();
        stride = pad + 1;
        const uint64_t total = (uint64_t)world * stride;
        if (stage.cap < total) {
            if (stage.d) (void)hipFree(stage.d);
            stage.d = nullptr, stage.cap = 0;
            uint64_t want = total + total / 2;
            hipError_t me = hipMalloc((void**)&stage.d, want * sizeof(double));
            if (me != hipSuccess) {  // without the headroom, then: what the exchange itself needs
                (void)hipGetLastError();
                want = total;
                me = hipMalloc((void**)&stage.d, want * sizeof(double));
            }
            // (no buffer at all: this rank has nothing to enter the in-place exchange with -- the one failure the status word cannot carry)
            if (me != hipSuccess) return localRc ? fail(localRc, ownError) : hipFail(me, "staging buffer of the exchange");
            stage.cap = want;
        }
        // a failing copy is this rank's failure like any other: it enters the exchange with its status set (the peers leave with
        // HPSDF_ERR_STATE instead of waiting for it in the next collective) and returns its own error afterwards
        if (count && !localRc) {
            const hipError_t ce = hipMemcpyAsync(stage.d + (uint64_t)rank * stride, mine, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
            if (ce != hipSuccess) localRc = hipFail(ce, "upload of this rank's part of the exchange"), ownError = hpsdf_last_error();
        }
        const double status = (double)localRc;
        {
            const hipError_t ce = hipMemcpyAsync(stage.d + (uint64_t)rank * stride + pad, &status, sizeof(double), hipMemcpyHostToDevice, ctx->stream);
            if (ce != hipSuccess && !localRc) localRc = hipFail(ce, "upload of this rank's status word"), ownError = hpsdf_last_error();
        }
        const int grc = gather(user, stage.d, stride * sizeof(double), (void*)ctx->stream);
        if (localRc) return fail(localRc, ownError);
        if (grc) return fail(HPSDF_ERR_STATE, std::string("the all-gather callback failed (") + what + "): " + std::to_string(grc));
        all.resize(total);
        HPSDF_HIP(hipMemcpyAsync(all.data(), stage.d, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HPSDF_HIP(hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < world; ++r)
            if (all[(uint64_t)r * stride + pad] != 0.0)
                return fail(HPSDF_ERR_STATE, "rank " + std::to_string(r) + " failed in this round (status " + std::to_string((int)all[(uint64_t)r * stride + pad]) +
                                                 ", " + what + "): its own error was returned there");
        return HPSDF_OK;
    }
};

// Create on the host scheduler, for what it owns (host callbacks, nearness weighting on several ranks, logging, K > 4096,
// HPSDF_HOST_FRONTIER=1): the round loop of hp-adaptive-..._amd/distributed.py in C++, for one rank or many.  Per round the ranks
// exchange the 9 errors of every job; for weighted builds also the arrays the round accepted (hpsdf_build_rows_*); at the end the
// packed coefficients.  begin(), then build(); the times are those of the HPSDF_TRACE line, which end() prints.
struct HostSchedulerCreate {
    hpsdf_ctx* ctx;
    const hpsdf_config* cfg;
    const hpsdf_field* field;
    int rank, world;
    RankExchange exchange;
    // whatever throws in a step (vector growth, std::thread creation in builderCompute ...), the build's destructor runs and
    // hands the context's workspace back (ws->inUse)
    std::unique_ptr<hpsdf_build> owner;
    std::vector<double> mine, headers;
    double tBegin = 0, tSel = 0, tCmp = 0, tRes = 0, tApp = 0, tLay = 0, tPack = 0, tAsm = 0, t0 = now(), tLap = t0;

    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    double lap() {  // the time since the last lap: the steps follow each other
        const double t = now(), d = t - tLap;
        tLap = t;
        return d;
    }

    int begin(uint64_t K) {
        hpsdf_build_opts o;
        std::memset(&o, 0, sizeof o);
        o.max_jobs_per_round = K;
        o.rank = rank;
        o.world = world;
        hpsdf_build* b = nullptr;
        const int rc = hpsdf_build_begin(cfg, &o, &b);
        if (rc) return rc;
        owner.reset(b);
        if (world > 1) HPSDF_HIP(hipSetDevice(ctx->device));  // (the exchange's staging buffer is this device's)
        tBegin = lap();
        return HPSDF_OK;
    }

    // select, compute, this rank's results, exchange, apply -- until a round selects nothing
    int rounds() {
        hpsdf_build* b = owner.get();
        std::vector<uint64_t> counts(world);
        std::vector<const double*> parts(world);
        for (;;) {
            uint64_t n = 0;
            int rc;
            if ((rc = builderSelect(b, &n))) return rc;
            tSel += lap();
            if (n == 0) return HPSDF_OK;
            // (this rank's share of the round: what can fail here fails on this rank alone -- the exchange carries the news)
            rc = builderCompute(b, ctx, field);
            tCmp += lap();
            const uint64_t myCount = b->slices[rank].count * HPSDF_JOB_HEADER_DOUBLES;
            uint64_t maxSlice = 0;
            for (const auto& sl : b->slices) maxSlice = std::max(maxSlice, sl.count);
            mine.resize(std::max<uint64_t>(1, myCount));
            if (!rc) rc = hpsdf_build_round_results_host(b, ctx, mine.data());
            const uint64_t pad = maxSlice * HPSDF_JOB_HEADER_DOUBLES;
            if ((rc = exchange(mine.data(), myCount, pad, "a round's errors", rc))) return rc;
            tRes += lap();
            const double* roundHeaders = exchange.part(0);  // (one rank: its slice is the round)
            if (world > 1) {
                headers.resize(n * HPSDF_JOB_HEADER_DOUBLES);
                for (int r = 0; r < world; ++r)
                    if (b->slices[r].count)
                        std::memcpy(headers.data() + b->slices[r].first * HPSDF_JOB_HEADER_DOUBLES, exchange.part(r),
                                    b->slices[r].count * HPSDF_JOB_HEADER_DOUBLES * sizeof(double));
                roundHeaders = headers.data();
            }
            if ((rc = builderApply(b, roundHeaders))) return rc;
            if (b->weighted && world > 1) {  // the arrays this round accepted go to every rank (Octree.cpp:847 copies a node's previous rows)
                if ((rc = builderRowsCounts(b, counts.data()))) return rc;
                uint64_t rpad = 0;
                for (uint64_t c : counts) rpad = std::max(rpad, c);
                if (rpad) {
                    mine.resize(std::max<uint64_t>(1, counts[rank]));
                    rc = builderRowsPackHost(b, ctx, mine.data());
                    if ((rc = exchange(mine.data(), counts[rank], rpad, "a round's accepted rows", rc))) return rc;
                    for (int r = 0; r < world; ++r) parts[r] = exchange.part(r);
                    if ((rc = builderRowsUnpackHost(b, ctx, parts.data()))) return rc;
                }
            }
            tApp += lap();
        }
    }

    // the rounds, then: layout, pack and exchange, assemble, adopt, stats
    int build(void** block, size_t* size, hpsdf_build_stats* stats) {
        int rc = rounds();
        if (rc) return rc;
        hpsdf_build* b = owner.get();
        if ((rc = builderLayout(b))) return rc;
        tLay = lap();
        uint64_t ppad = 1;
        for (uint64_t c : b->packCounts) ppad = std::max(ppad, c);
        mine.resize(std::max<uint64_t>(1, b->packCounts[rank]));
        rc = builderPackHost(b, ctx, mine.data());
        if ((rc = exchange(mine.data(), b->packCounts[rank], ppad, "the packed coefficients", rc))) return rc;
        tPack = lap();
        std::vector<const double*> parts(world);
        for (int r = 0; r < world; ++r) parts[r] = exchange.part(r);
        if ((rc = builderAssemble(b, parts.data(), block, size))) return rc;
        if ((rc = adoptBlock(ctx, block, *size))) return rc;
        tAsm = lap();
        if (stats) hpsdf_build_get_stats(b, stats);
        return HPSDF_OK;
    }

    // hpsdf_create's last step, after its continuity pass: the build goes, and HPSDF_TRACE gets its line (tools/create_trace.py reads it)
    void end() {
        const double tCont = lap();
        owner.reset();
        if (std::getenv("HPSDF_TRACE") != nullptr)
            std::fprintf(stderr, "[hpsdf_create] us: begin %.0f select %.0f compute(host+launch) %.0f results(wait+D2H) %.0f apply %.0f "
                                 "layout %.0f pack %.0f assemble %.0f continuity %.0f destroy %.0f total %.0f\n",
                         tBegin, tSel, tCmp, tRes, tApp, tLay, tPack, tAsm, tCont, lap(), now() - t0);
    }
};

}  // namespace

extern "C" {

int hpsdf_create(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, uint64_t K, void** block,
                 size_t* size, hpsdf_build_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "Create runs on the GPU: a device context is required");
    if (!cfg || !field || !block || !size) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (frontierEligible(ctx, cfg, field, K))  // frontier, decision and bookkeeping on the device (frontier.hip)
        return continuityAfterCreate(ctx, cfg, block, size, frontierCreate(ctx, cfg, field, K, block, size, stats));
    HostSchedulerCreate hs{ctx, cfg, field, 0, 1, {ctx, 0, 1, nullptr, nullptr}};
    int rc = hs.begin(K);
    if (rc) return rc;
    rc = continuityAfterCreate(ctx, cfg, block, size, hs.build(block, size, stats));
    hs.end();
    return rc;
    HPSDF_CATCH
}

int hpsdf_create_distributed(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, uint64_t K, int rank, int world,
                             hpsdf_allgather_fn gather, void* user, void** block, size_t* size, hpsdf_build_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "Create runs on the GPU: a device context is required");
    if (!cfg || !field || !block || !size) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (world == 1) return hpsdf_create(ctx, cfg, field, K, block, size, stats);
    if (world < 1 || rank < 0 || rank >= world) return fail(HPSDF_ERR_INVALID_ARGUMENT, "rank outside [0, world)");
    if (!gather) return fail(HPSDF_ERR_INVALID_ARGUMENT, "an all-gather callback is required for world > 1");
    // (the device-side frontier packs a segment's owner rank into three bits: more than 8 ranks take the host scheduler's rounds)
    // (... and a weighted incremental fit needs the node's previous rows, which another rank may hold: the host scheduler's
    // sharded rounds hand them over)
    int rc;
    if (frontierEligible(ctx, cfg, field, K) && world <= 8) {
        rc = frontierCreate(ctx, cfg, field, K, block, size, stats, rank, world, gather, user);
    } else {
        HostSchedulerCreate hs{ctx, cfg, field, rank, world, {ctx, rank, world, gather, user}};
        if (!(rc = hs.begin(K))) rc = hs.build(block, size, stats);
    }  // (the build is gone before the continuity pass)
    return continuityAfterCreate(ctx, cfg, block, size, rc);
    HPSDF_CATCH
}

// ---------------------------------------------------------------------------- continuity (host)
int hpsdf_continuity_post_process(void* block, size_t size, double tol, int maxIter, uint64_t threads,
                                  hpsdf_continuity_stats* stats) {
    HPSDF_TRY
    std::string err;
    const int rc = continuityPostProcess(block, size, tol, maxIter, threads, stats, err);
    if (rc) return fail(rc, err);
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_continuity_post_process_device(hpsdf_ctx* ctx, void* block, size_t size, double tol, int maxIter, uint64_t threads,
                                         hpsdf_continuity_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required (hpsdf_continuity_post_process solves on the host)");
    std::string err;
    const int rc = continuityPostProcess(block, size, tol, maxIter, threads, stats, err, ctx);
    if (rc) return fail(rc, err);
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_continuity_matrix(const void* block, size_t size, uint64_t threads, uint64_t** rowPtr, uint64_t** col,
                            double** val, hpsdf_continuity_stats* stats) {
    HPSDF_TRY
    if (!rowPtr || !col || !val) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null output");
    std::string err;
    const int rc = continuityMatrix(block, size, threads, rowPtr, col, val, stats, err);
    if (rc) return fail(rc, err);
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_continuity_matrix_device(hpsdf_ctx* ctx, const void* block, size_t size, uint64_t** rowPtr, uint64_t** col, double** val,
                                   hpsdf_continuity_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!block || !rowPtr || !col || !val) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    std::string err;
    const int rc = continuityMatrixDevice(ctx, block, size, rowPtr, col, val, stats, err);
    if (rc) return fail(rc, err);
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_continuity_last_stats(hpsdf_continuity_stats* out) {
    if (!out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null out");
    *out = g_lastContinuity;
    return HPSDF_OK;
}

}  // extern "C"
