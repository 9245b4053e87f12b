// C ABI of include/hpsdf.h: the error state, the process-wide settings, the build-limit policy and the contexts.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>

#include "launch.hpp"
#include "runtime.hpp"

using namespace hpsdf;

namespace hpsdf {

static thread_local std::string g_lastError;

void setError(const std::string& msg) { g_lastError = msg; }
int fail(int code, const std::string& msg) {
    g_lastError = msg;
    return code;
}
int hipFail(hipError_t e, const char* what) {
    g_lastError = std::string(what) + ": " + hipGetErrorString(e);
    // the runtime keeps a failed call's code as its "last error" until somebody asks for it: taken here, so that the launch checks of the
    // NEXT call (hipGetLastError() behind every kernel launch) do not report this call's failure again (seen in tools/fuzz_split.py: the
    // build after one that ran out of memory was refused with "launch of fr_init_kernel: out of memory")
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? HPSDF_ERR_NO_DEVICE
                                                                                                 : HPSDF_ERR_HIP;
}

const hpsdf_field* innermost(const hpsdf_field* f) {
    while (f && f->kind == kHostTreeCsg) f = f->inner;
    return f;
}

static int envLeftAssoc() {
    const char* e = std::getenv("HPSDF_REDUCTION_ORDER");  // "left" / "1": (a . b) . c from the start
    return e && (e[0] == 'l' || e[0] == 'L' || e[0] == '1');
}
static std::atomic<int> gLeftAssoc{envLeftAssoc()};
int reductionLeftAssoc(const hpsdf_ctx* ctx) { return ctx && ctx->reductionOrder >= 0 ? ctx->reductionOrder : gLeftAssoc.load(std::memory_order_relaxed); }
void setReductionLeftAssoc(int left) { gLeftAssoc.store(left != 0, std::memory_order_relaxed); }

// hpsdf_set_mesh_face_rule(): 0 = a face-case point that has left its triangle is replaced by the boundary's closest point (default: every
// evaluation path then gives one answer), 1 = the reference's point whatever its weights (Source/Meshing/Utility.cpp:5-97)
static int envMeshFaceRule() {
    const char* e = std::getenv("HPSDF_MESH_FACE_RULE");  // "reference" / "1"
    return e && (e[0] == 'r' || e[0] == 'R' || e[0] == '1');
}
static std::atomic<int> gMeshFaceReference{envMeshFaceRule()};
int meshFaceRuleReference(const hpsdf_ctx* ctx) { return ctx && ctx->meshFaceRule >= 0 ? ctx->meshFaceRule : gMeshFaceReference.load(std::memory_order_relaxed); }
void setMeshFaceRuleReference(int on) { gMeshFaceReference.store(on != 0, std::memory_order_relaxed); }
float meshFaceTolOfSlack(const hpsdf_ctx* ctx) { return meshFaceRuleReference(ctx) ? std::numeric_limits<float>::infinity() : 0.25f; }

uint64_t buildByteLimit(const hpsdf_ctx* ctx, uint64_t growBytes, uint64_t held, uint64_t* measured) {
    constexpr uint64_t kNone = ~0ull, kMeasureFrom = 256ull << 20;
    if (ctx->limitBytes) return ctx->limitBytes;
    if (growBytes <= kMeasureFrom) return kNone;  // (nothing is measured for builds that stay small: every BASELINE config)
    if (*measured == 0) {  // the default: 1/64 of what the device could give this build, at least 1 GiB
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) {
            (void)hipGetLastError();
            freeB = 0;
        }
        *measured = std::max<uint64_t>(1ull << 30, ((uint64_t)freeB + held) / 64);
    }
    return *measured;
}
// bytes: everything the round about to open needs on the device; growBytes: the part of it that grows with the tree (nodes, coefficient
// arena).  A limit the caller set bounds `bytes`.  The DEFAULT exists to end a build that will not end by itself (the reference's default
// Config()) in seconds instead of minutes, and bounds `growBytes` only: a round's sample buffer -- a mesh field's, K x up to 150 000
// samples a job, at most 2^31 samples = 16 GiB whatever the tree's size -- is what an ordinary mesh build at K = 4096 needs (2.9 GiB at
// degree 4) and says nothing about whether the build runs away.  (1/64: 4.5 GiB on an idle MI355X, a tree of some 10 M nodes; at 1/256 a
// mesh build at 1e-8 that was two thirds of the way to its threshold with 3.7 M nodes was refused.)
int checkBuildLimits(const hpsdf_ctx* ctx, uint64_t nodes, uint64_t bytes, uint64_t growBytes, uint64_t held, uint64_t* measured, uint64_t rounds, double total, double target) {
    constexpr uint64_t kNone = ~0ull;
    const uint64_t maxNodes = ctx->limitNodes ? ctx->limitNodes : kNone;
    const uint64_t maxBytes = buildByteLimit(ctx, growBytes, held, measured);
    const uint64_t counted = ctx->limitBytes ? bytes : growBytes;
    const char* how = ctx->limitBytes ? "hpsdf_ctx_set_build_limits" : "the default, on nodes and coefficients: 1/64 of the device memory that was free, at least 1 GiB";
    if (nodes <= maxNodes && counted <= maxBytes) return HPSDF_OK;
    char msg[704];
    std::snprintf(msg, sizeof msg,
                  "build limit: after %llu rounds the tree has %llu nodes (limit %s%llu) and the next round needs %.3f GiB of device memory (limit %.3f GiB, %s); "
                  "total error %.3e against the threshold %.3e -- the threshold may be below what the error estimate reaches on this field. "
                  "hpsdf_ctx_set_build_limits(ctx, max_nodes, max_bytes) raises the limits (UINT64_MAX: none)",
                  (unsigned long long)rounds, (unsigned long long)nodes, maxNodes == kNone ? "none, " : "", (unsigned long long)(maxNodes == kNone ? 0 : maxNodes),
                  (double)counted / (double)(1ull << 30), maxBytes == kNone ? 0.0 : (double)maxBytes / (double)(1ull << 30), maxBytes == kNone ? "none" : how, total, target);
    return fail(HPSDF_ERR_BUILD_LIMIT, msg);
}

int makeFieldDev(const hpsdf_ctx* ctx, const hpsdf_field* f, const double* dSamples, FieldDev* out) {
    std::memset(out, 0, sizeof(*out));
    out->csgOp = -1;
    if (f->kind == kHostTreeCsg) {
        if (!f->oldTree || !f->inner) return fail(HPSDF_ERR_INVALID_ARGUMENT, "csg field without tree or inner field");
        if (f->inner->kind == kHostTreeCsg) return fail(HPSDF_ERR_UNSUPPORTED, "nested csg fields are not supported");
        out->csgOp = f->csgOp;
        out->oldTree = f->oldTree->dev;
        f = f->inner;
    }
    switch (f->kind) {
        case kHostAnalytic:
            out->kind = kFieldAnalytic;
            out->nPrims = (int32_t)f->prims.size();
            for (size_t i = 0; i < f->prims.size(); ++i) out->prims[i] = f->prims[i];
            break;
        case kHostCallback:
            out->kind = kFieldSamples;
            out->samples = dSamples;
            break;
        case kHostMesh:
            out->kind = kFieldMesh;
            out->mesh.verts = f->dVerts;
            out->mesh.tris = f->dTris;
            out->mesh.halfEdges = f->dHalfEdges;
            out->mesh.triPos = reinterpret_cast<const float4*>(f->dTriPos);
            out->mesh.triPre = reinterpret_cast<const float4*>(f->dTriPre);
            out->mesh.bvh = f->dBvh;
            out->mesh.slabs = f->dSlabs;
            out->mesh.leafLog2 = f->leafLog2;
            {
                const char* pc = std::getenv("HPSDF_MESH_POOL_CAP");  // tests: a small pool sends lanes through the overflow path
                out->mesh.poolCap = pc ? (uint32_t)std::strtoul(pc, nullptr, 10) : 0xFFFFFFFFu;
            }
            out->mesh.nTris = f->nTris;
            out->mesh.nNodes = f->nBvhNodes;
            out->mesh.stats = f->dStats;
            out->mesh.faceTolOfSlack = meshFaceTolOfSlack(ctx);
            break;
        default:
            return fail(HPSDF_ERR_INVALID_ARGUMENT, "unknown field kind");
    }
    out->leftAssoc = reductionLeftAssoc(ctx);
    return HPSDF_OK;
}

}  // namespace hpsdf

extern "C" {

const char* hpsdf_last_error(void) { return g_lastError.c_str(); }
const char* hpsdf_version(void) { return "hpsdf-gfx950 0.4"; }  // (minor = HPSDF_ABI_VERSION)
int hpsdf_abi_version(void) { return HPSDF_ABI_VERSION; }

int hpsdf_config_default(hpsdf_config* c) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null config");
    std::memset(c, 0, sizeof(*c));
    c->target_error_threshold = std::pow(10, -10);
    c->weighting_type = 0;
    c->continuity_enforce = 1;
    c->continuity_strength = 8.0;
    const unsigned hc = std::thread::hardware_concurrency();
    c->thread_count = hc ? hc : 1;
    for (int a = 0; a < 3; ++a) {
        c->root_min[a] = -0.5f;
        c->root_max[a] = 0.5f;
    }
    return HPSDF_OK;
}

int hpsdf_tables_get(double* roots, double* weights, double* nl, double* rec, uint64_t* count, uint64_t* bidx,
                     uint64_t* sumToN) {
    HPSDF_TRY
    const Tables& T = tables();
    if (roots) std::memcpy(roots, T.roots, sizeof T.roots);
    if (weights) std::memcpy(weights, T.weights, sizeof T.weights);
    if (nl) std::memcpy(nl, T.normalisedLengths, sizeof T.normalisedLengths);
    if (rec) std::memcpy(rec, T.recurrence, sizeof T.recurrence);
    if (count) std::memcpy(count, T.coeffCount, sizeof T.coeffCount);
    if (bidx) std::memcpy(bidx, T.basisIndex, sizeof T.basisIndex);
    if (sumToN) std::memcpy(sumToN, T.sumToN, sizeof T.sumToN);
    return HPSDF_OK;
    HPSDF_CATCH
}

// ---------------------------------------------------------------------------- context
int hpsdf_ctx_create(int device, void* stream, hpsdf_ctx** out) {
    HPSDF_TRY
    if (!out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(HPSDF_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0"));
    if (device < 0 || device >= n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    HPSDF_HIP(hipSetDevice(device));
    hpsdf_ctx* c = new hpsdf_ctx();
    c->device = device;
    c->splitMinDegree = fitSplitDefaultMinDegree();
    if (const char* fm = std::getenv("HPSDF_FIT_MODE")) {  // the mode a context starts with (hpsdf_ctx_set_fit_mode changes it)
        if (!std::strcmp(fm, "exact")) c->fitMode = HPSDF_FIT_EXACT;
        else if (!std::strcmp(fm, "fast")) c->fitMode = HPSDF_FIT_FAST;
        else if (!std::strcmp(fm, "split")) c->fitMode = HPSDF_FIT_SPLIT;
    }
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete c;
            return hipFail(se, "hipStreamCreate");
        }
        c->ownsStream = true;
    }
    // constant tables -> HBM
    const Tables& T = tables();
    DeviceTables* h = new DeviceTables();
    std::memset(h, 0, sizeof(*h));
    std::memcpy(h->roots, T.roots, sizeof T.roots);
    std::memcpy(h->weights, T.weights, sizeof T.weights);
    std::memcpy(h->nl, T.normalisedLengths, sizeof T.normalisedLengths);
    std::memcpy(h->rec, T.recurrence, sizeof T.recurrence);
    for (int i = 0; i < kMaxCoeffs; ++i) {
        h->bidx[i][0] = (uint8_t)T.basisIndex[i][0];
        h->bidx[i][1] = (uint8_t)T.basisIndex[i][1];
        h->bidx[i][2] = (uint8_t)T.basisIndex[i][2];
        h->bidx[i][3] = (uint8_t)(T.basisIndex[i][0] + T.basisIndex[i][1] + T.basisIndex[i][2]);
    }
    for (int i = 0; i <= kMaxDegree; ++i) h->count[i] = (uint32_t)T.coeffCount[i];
    std::memcpy(h->transfer, T.transfer, sizeof T.transfer);
    hipError_t me = hipMalloc((void**)&c->dTables, sizeof(DeviceTables));
    if (me == hipSuccess) me = hipMemcpy(c->dTables, h, sizeof(DeviceTables), hipMemcpyHostToDevice);
    delete h;
    if (me != hipSuccess) {
        hpsdf_ctx_destroy(c);
        return hipFail(me, "table upload");
    }
    *out = c;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_ctx_destroy(hpsdf_ctx* c) {
    if (!c) return HPSDF_OK;
    (void)hipSetDevice(c->device);
    // (nothing of this context's may still be running when its buffers go: a build leaves its tables' reset on the stream for the next
    // one, and pinned host memory the device writes -- the header's mirror -- is freed below)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    if (c->dTables) (void)hipFree(c->dTables);
    if (c->hostDev) (void)hipFree(c->hostDev);
    if (c->hostPin) (void)hipHostFree(c->hostPin);
    if (c->dDefer) (void)hipFree(c->dDefer);
    if (c->dDeferCount) (void)hipFree(c->dDeferCount);
    c->ws.release();
    if (c->ownsStream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return HPSDF_OK;
}

int hpsdf_ctx_set_stream(hpsdf_ctx* c, void* stream) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null ctx");
    hipStream_t next = (hipStream_t)stream;
    if (next == c->stream) return HPSDF_OK;  // (also the owned stream handed back: it stays, and stays owned)
    HPSDF_HIP(hipSetDevice(c->device));
    if (c->ownsStream && c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
        c->ownsStream = false;
    } else {
        // What the context has queued on the caller's old stream may still be running, on scratch that its next call shares (Query's
        // deferred lists, the *_host entries' buffers, the build's workspace): the new stream starts behind it.  No host wait.
        hipEvent_t done = nullptr;
        HPSDF_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        hipError_t e = hipEventRecord(done, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(next, done, 0);
        (void)hipEventDestroy(done);  // (released once the wait has been served)
        if (e != hipSuccess) return hipFail(e, "hpsdf_ctx_set_stream: ordering the new stream behind the old one");
    }
    c->stream = next;
    return HPSDF_OK;
}

int hpsdf_ctx_set_fit_mode(hpsdf_ctx* c, int mode) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    if (mode != HPSDF_FIT_EXACT && mode != HPSDF_FIT_SPLIT && mode != HPSDF_FIT_FAST) return fail(HPSDF_ERR_INVALID_ARGUMENT, "unknown fit mode");
    c->fitMode = mode;
    return HPSDF_OK;
}
int hpsdf_ctx_get_fit_mode(hpsdf_ctx* c, int* mode) {
    if (!c || !mode) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *mode = c->fitMode;
    return HPSDF_OK;
}
int hpsdf_ctx_set_build_limits(hpsdf_ctx* c, uint64_t max_nodes, uint64_t max_bytes) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    c->limitNodes = max_nodes, c->limitBytes = max_bytes;
    return HPSDF_OK;
}
int hpsdf_ctx_get_build_limits(const hpsdf_ctx* c, uint64_t* max_nodes, uint64_t* max_bytes) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    if (max_nodes) *max_nodes = c->limitNodes;
    if (max_bytes) *max_bytes = c->limitBytes;
    return HPSDF_OK;
}
int hpsdf_ctx_set_split_min_degree(hpsdf_ctx* c, int degree) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    if (degree < 2 || degree > 12) return fail(HPSDF_ERR_INVALID_ARGUMENT, "split_min_degree: 2..12 (12 = never split)");
    c->splitMinDegree = degree;
    return HPSDF_OK;
}
void hpsdf_set_mesh_face_rule(int reference) { setMeshFaceRuleReference(reference); }
int hpsdf_get_mesh_face_rule(void) { return meshFaceRuleReference(nullptr); }
void hpsdf_set_reduction_order(int left_assoc) { setReductionLeftAssoc(left_assoc); }
int hpsdf_get_reduction_order(void) { return reductionLeftAssoc(nullptr); }
// per context (-1: follow the process-wide setting above)
int hpsdf_ctx_set_reduction_order(hpsdf_ctx* c, int left_assoc) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    if (left_assoc < -1 || left_assoc > 1) return fail(HPSDF_ERR_INVALID_ARGUMENT, "reduction order: -1 (the process-wide setting), 0 or 1");
    c->reductionOrder = left_assoc;
    return HPSDF_OK;
}
int hpsdf_ctx_get_reduction_order(const hpsdf_ctx* c, int* left_assoc) {
    if (!c || !left_assoc) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *left_assoc = reductionLeftAssoc(c);
    return HPSDF_OK;
}
int hpsdf_ctx_set_mesh_face_rule(hpsdf_ctx* c, int reference) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null context");
    if (reference < -1 || reference > 1) return fail(HPSDF_ERR_INVALID_ARGUMENT, "mesh face rule: -1 (the process-wide setting), 0 or 1");
    c->meshFaceRule = reference;
    return HPSDF_OK;
}
int hpsdf_ctx_get_mesh_face_rule(const hpsdf_ctx* c, int* reference) {
    if (!c || !reference) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *reference = meshFaceRuleReference(c);
    return HPSDF_OK;
}
int hpsdf_ctx_set_fast_fit(hpsdf_ctx* c, int on) { return hpsdf_ctx_set_fit_mode(c, on ? HPSDF_FIT_FAST : HPSDF_FIT_EXACT); }

int hpsdf_ctx_synchronize(hpsdf_ctx* c) {
    if (!c) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null ctx");
    HPSDF_HIP(hipSetDevice(c->device));
    HPSDF_HIP(hipStreamSynchronize(c->stream));
    return HPSDF_OK;
}

void* hpsdf_ctx_stream(hpsdf_ctx* c) { return c ? (void*)c->stream : nullptr; }

void hpsdf_ctx_set_block_allocator(hpsdf_ctx* ctx, hpsdf_block_alloc_fn alloc, hpsdf_block_release_fn release, void* user) {
    if (!ctx) return;
    ctx->blockAlloc = alloc, ctx->blockRelease = alloc ? release : nullptr, ctx->blockUser = alloc ? user : nullptr;
}

}  // extern "C"
