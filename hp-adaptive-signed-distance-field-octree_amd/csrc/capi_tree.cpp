// C ABI of include/hpsdf.h: the tree upload and every query entry over a tree, _device and _host, with the slice renderer.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "block.hpp"
#include "clearance.hpp"
#include "host_call.hpp"
#include "integrate.hpp"
#include "integrate_pair.hpp"
#include "launch.hpp"
#include "ray_cast.hpp"
#include "runtime.hpp"
#include "simplify.hpp"
#include "tree_bound.hpp"

using namespace hpsdf;

namespace {
// "This tree on this context, ready to launch", the prologue of the *_device entries that take a tree: a tree of another device is refused,
// the context's device becomes the current one, *td (if asked for) is the tree as the kernels take it, in the context's reduction order.
int treeOnContext(hpsdf_ctx* ctx, const hpsdf_tree* t, TreeDev* td = nullptr) {
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    HPSDF_HIP(hipSetDevice(ctx->device));
    if (td) *td = t->dev, td->leftAssoc = reductionLeftAssoc(ctx);
    return HPSDF_OK;
}
// This tree as the bounds and the integral walk it (tree_bound.hpp): over its device arrays (boundConsts() made), and over its host
// copies (hostCopies() and boundHostCopies() made)
ClsTree clsTreeOnDevice(const hpsdf_tree* t) {
    const double *c = t->dev.rootCentre, *s = t->dev.rootInvSizes;
    return ClsTree{t->dev.nodes, t->dev.coeffs, t->dBoundConsts, {c[0], c[1], c[2]}, {s[0], s[1], s[2]}};
}
ClsTree clsTreeOnHost(const hpsdf_tree* t) {
    const double *c = t->dev.rootCentre, *s = t->dev.rootInvSizes;
    return ClsTree{t->hRecs.data(), t->hPadded.data(), t->hBoundConsts.data(), {c[0], c[1], c[2]}, {s[0], s[1], s[2]}};
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------- tree + query
int hpsdf_tree_upload(hpsdf_ctx* ctx, const void* block, size_t size, hpsdf_tree** out) {
    HPSDF_TRY
    if (!out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "trees are queried on the GPU: a device context is required");
    const Tables& T = tables();
    BlockView v;
    BlockMirror m;
    {
        std::string why;
        int rc = readBlock(block, size, v, why);
        if (!rc) rc = mirrorBlock(v, T, m, why);  // validates that the tree is the dyadic octree the descent recomputes
        if (rc) return fail(rc, why);
    }
    // dense table of the deepest complete level (<= 5): table[path] = node reached by that octant path
    const int topDepth = std::max(1, std::min(5, m.walk.minLeafDepth));
    std::vector<TopEntry> top((size_t)1 << (3 * topDepth));
    std::vector<NodeRec> topRec(top.size());
    for (size_t code = 0; code < top.size(); ++code) {  // code = x + side * (y + side * z), cell coordinates at topDepth
        const size_t mask = ((size_t)1 << topDepth) - 1;
        const size_t kx = code & mask, ky = (code >> topDepth) & mask, kz = code >> (2 * topDepth);
        uint64_t cur = 0;
        for (int l = topDepth - 1; l >= 0; --l)  // bit l of a coordinate picks the upper half at that level (Octree.cpp:1101)
            cur = v.nodes[cur].child_idx + ((kx >> l) & 1u) + 2 * ((ky >> l) & 1u) + 4 * ((kz >> l) & 1u);
        TopEntry& te = top[code];
        std::memset(&te, 0, sizeof te);
        te.a = m.recs[cur].a;
        te.b = m.recs[cur].b;
        topRec[code] = m.recs[cur];
        if (te.b <= 2u)  // small leaf: coefficients ride in the same line
            std::memcpy(te.c, v.coeffs + v.nodes[cur].coeffs_start, sizeof(double) * T.coeffCount[te.b]);
    }
    HPSDF_HIP(hipSetDevice(ctx->device));
    hpsdf_tree* t = new hpsdf_tree();
    t->device = ctx->device;
    t->nNodes = v.nNodes;
    t->nCoeffs = v.nCoeffs;
    t->nLeaves = m.walk.leaves;
    t->maxDegree = m.walk.maxDegree;
    t->maxDepth = m.walk.maxDepth;
    t->allInline = m.walk.maxDegree <= 2 && m.walk.maxDepth <= topDepth;
    t->config = v.cfg;
    hipError_t e = hipMalloc((void**)&t->dNodes, v.nNodes * sizeof(NodeRec));
    if (e == hipSuccess) e = hipMalloc((void**)&t->dCoeffs, std::max<size_t>(2, m.padded.size()) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&t->dTop, top.size() * sizeof(TopEntry));
    if (e == hipSuccess) e = hipMalloc((void**)&t->dTopRec, topRec.size() * sizeof(NodeRec));
    if (e == hipSuccess) e = hipMemcpy(t->dTopRec, topRec.data(), topRec.size() * sizeof(NodeRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->dNodes, m.recs.data(), v.nNodes * sizeof(NodeRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->dTop, top.data(), top.size() * sizeof(TopEntry), hipMemcpyHostToDevice);
    if (e == hipSuccess && !m.padded.empty())
        e = hipMemcpy(t->dCoeffs, m.padded.data(), m.padded.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hpsdf_tree_destroy(t);
        return hipFail(e, "tree upload");
    }
    t->dev.nodes = t->dNodes;
    t->dev.top = t->dTop;
    t->dev.topRec = t->dTopRec;
    t->dev.coeffs = t->dCoeffs;
    t->dev.topDepth = topDepth;
    t->dev.maxDegree = m.walk.maxDegree;
    for (int j = 0; j < 3; ++j) t->dev.nlTop[j] = T.normalisedLengths[j][topDepth];
    for (int a = 0; a < 3; ++a) t->dev.rootCentre[a] = m.rootCentre[a], t->dev.rootInvSizes[a] = m.rootInvSizes[a];
    t->paddedCount = m.padded.size();
    *out = t;
    return HPSDF_OK;
    HPSDF_CATCH
}

// The host copies a scalar-sized call works from (host_query.cpp), on first use: the device mirror's records and coefficients.
int hpsdf_tree::hostCopies() const {
    if (hostReady.load(std::memory_order_acquire)) return HPSDF_OK;
    std::lock_guard<std::mutex> guard(hostLock);
    if (hostReady.load(std::memory_order_relaxed)) return HPSDF_OK;
    HPSDF_HIP(hipSetDevice(device));
    hRecs.resize(nNodes);
    hPadded.resize(std::max<uint64_t>(2, paddedCount));
    HPSDF_HIP(hipMemcpy(hRecs.data(), dNodes, nNodes * sizeof(hpsdf::NodeRec), hipMemcpyDeviceToHost));  // (the upload's copies were synchronous)
    if (paddedCount) HPSDF_HIP(hipMemcpy(hPadded.data(), dCoeffs, paddedCount * sizeof(double), hipMemcpyDeviceToHost));
    hostReady.store(true, std::memory_order_release);
    return HPSDF_OK;
}

int hpsdf_tree_destroy(hpsdf_tree* t) {
    if (!t) return HPSDF_OK;
    (void)hipSetDevice(t->device);
    if (t->dNodes) (void)hipFree(t->dNodes);
    if (t->dTop) (void)hipFree(t->dTop);
    if (t->dTopRec) (void)hipFree(t->dTopRec);
    if (t->dCoeffs) (void)hipFree(t->dCoeffs);
    if (t->dBoundConsts) (void)hipFree(t->dBoundConsts);
    if (t->dLeafCells) (void)hipFree(t->dLeafCells);
    delete t;
    return HPSDF_OK;
}

int hpsdf_tree_info(const hpsdf_tree* t, uint64_t* nNodes, uint64_t* nCoeffs, uint64_t* nLeaves, int* maxDegree,
                    int* maxDepth) {
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (nNodes) *nNodes = t->nNodes;
    if (nCoeffs) *nCoeffs = t->nCoeffs;
    if (nLeaves) *nLeaves = t->nLeaves;
    if (maxDegree) *maxDegree = t->maxDegree;
    if (maxDepth) *maxDepth = t->maxDepth;
    return HPSDF_OK;
}

// Query / QueryWithGradient over device arrays (dGrad == nullptr: values only)
static int queryDevice(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, double* dOut, double* dGrad) {
    TreeDev td;
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    const size_t kChunk = (size_t)1 << 31;  // deferred indices are 32-bit
    for (size_t off = 0; off < n; off += kChunk) {
        const size_t m = std::min(kChunk, n - off);
        // Query* is const and callable from many threads in the reference (Octree.h:71-78): the deferred-point scratch is
        // the one piece of context state these entry points touch -- grown and handed to the launch under one lock
        // (launches on the context stream run in order, so sharing the buffer between them is safe)
        std::unique_lock<std::mutex> guard(ctx->scratchLock, std::defer_lock);
        if (t->maxDegree > 3) {
            guard.lock();
            if (!ctx->dDeferCount) HPSDF_HIP(hipMalloc((void**)&ctx->dDeferCount, (2 * kQueryMaxGrid + 1) * sizeof(uint32_t)));
            const size_t need = m + (size_t)256 * kQueryMaxGrid + 4096;  // every workgroup's run is whole tiles
            if (ctx->deferCap < need) {
                if (ctx->dDefer) HPSDF_HIP(hipFree(ctx->dDefer));
                ctx->dDefer = nullptr;
                ctx->deferCap = 0;
                HPSDF_HIP(hipMalloc((void**)&ctx->dDefer, need * sizeof(uint32_t)));
                ctx->deferCap = need;
            }
        }
        HPSDF_HIP(launchQuery(ctx->stream, td, ctx->dTables, dXyz + 3 * off, m, dOut + off, dGrad ? dGrad + 3 * off : nullptr,
                              t->allInline, ctx->dDeferCount, ctx->dDefer));
    }
    return HPSDF_OK;
}

int hpsdf_query_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, double* dOut) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (!dXyz && n) || (!dOut && n)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return queryDevice(ctx, t, dXyz, n, dOut, nullptr);
    HPSDF_CATCH
}

int hpsdf_query_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (!xyz && n) || (!out && n)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n <= hostQueryLimit() && smallQueriesOnHost()) {  // a scalar Query(pt): ~0.05 us here, ~15 us as a launch (host_query.cpp)
        if (const int hc = t->hostCopies()) return hc;
        for (size_t i = 0; i < n; ++i) out[i] = hostQueryPoint(*t, xyz + 3 * i);
        return HPSDF_OK;
    }
    return hostRoundTrip(ctx, xyz, n, out, [&](const double* d, double* r) { return hpsdf_query_device(ctx, t, d, n, r); });
    HPSDF_CATCH
}

int hpsdf_query_gradient_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, double* dOut,
                                double* dGrad) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (n && (!dXyz || !dOut || !dGrad))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return queryDevice(ctx, t, dXyz, n, dOut, dGrad);
    HPSDF_CATCH
}

int hpsdf_query_gradient_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double* out,
                              double* grad) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (n && (!xyz || !out || !grad))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    if (n <= hostGradientLimit() && smallQueriesOnHost()) {
        if (const int hc = t->hostCopies()) return hc;
        for (size_t i = 0; i < n; ++i) hostQueryPointWithGradient(*t, xyz + 3 * i, out + i, grad + 3 * i, reductionLeftAssoc(ctx));
        return HPSDF_OK;
    }
    // rows of points outside the root keep what the caller passed in (the reference leaves its output untouched)
    HostArrays arr;
    const auto dXyz = arr.in(xyz, n * 3);
    const auto dOut = arr.out(out, n);
    const auto dGrad = arr.inout(grad, n * 3);
    return hostCall(ctx, arr, [&] { return hpsdf_query_gradient_device(ctx, t, dXyz, n, dOut, dGrad); });
    HPSDF_CATCH
}

// QueryGradient (include/hpsdf.h): the value and the gradient of the polynomial it comes from (query_gradient.hip, host_query.cpp)
int hpsdf_query_true_gradient_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, uint32_t flags, double* dOut,
                                     double* dGrad) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (flags & ~HPSDF_GRADIENT_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_true_gradient: unknown flag bits");
    if (!t || (n && (!dXyz || !dGrad))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    TreeDev td;
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    HPSDF_HIP(launchQueryTrueGradient(ctx->stream, td, ctx->dTables, dXyz, n, flags, dOut, dGrad, t->allInline));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_query_true_gradient_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, uint32_t flags, double* out,
                                   double* grad) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (flags & ~HPSDF_GRADIENT_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_true_gradient: unknown flag bits");
    if (!t || (n && (!xyz || !grad))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    if (n <= kHostQueryPoints && smallQueriesOnHost()) {
        if (const int hc = t->hostCopies()) return hc;
        hostTrueGradientRows(*t, xyz, n, flags, reductionLeftAssoc(ctx), out, grad);
        return HPSDF_OK;
    }
    HostArrays arr;
    const auto dXyz = arr.in(xyz, n * 3);
    const auto dOut = arr.out(out, n);
    const auto dGrad = arr.out(grad, n * 3);
    return hostCall(ctx, arr, [&] { return hpsdf_query_true_gradient_device(ctx, t, dXyz, n, flags, dOut, dGrad); });
    HPSDF_CATCH
}

// QueryHessian (include/hpsdf.h): value, gradient, second derivative and level-set curvature (query_hessian.hip, host_query.cpp)
int hpsdf_query_hessian_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, uint32_t flags, double* dOut, double* dGrad,
                               double* dHess, double* dCurv) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = hessianArgumentError(flags, dXyz, n, dHess, dCurv)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    TreeDev td;
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    HPSDF_HIP(launchQueryHessian(ctx->stream, td, ctx->dTables, dXyz, n, flags, dOut, dGrad, dHess, dCurv));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_query_hessian_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, uint32_t flags, double* out, double* grad,
                             double* hess, double* curv) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = hessianArgumentError(flags, xyz, n, hess, curv)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    if (n <= kHostQueryPoints && smallQueriesOnHost()) {
        if (const int hc = t->hostCopies()) return hc;
        hostHessianRows(*t, xyz, n, flags, reductionLeftAssoc(ctx), out, grad, hess, curv);
        return HPSDF_OK;
    }
    HostArrays arr;
    const auto dXyz = arr.in(xyz, n * 3);
    const auto dOut = arr.out(out, n);
    const auto dGrad = arr.out(grad, n * 3);
    const auto dHess = arr.out(hess, n * 6);
    const auto dCurv = arr.out(curv, n * 2);
    return hostCall(ctx, arr, [&] { return hpsdf_query_hessian_device(ctx, t, dXyz, n, flags, dOut, dGrad, dHess, dCurv); });
    HPSDF_CATCH
}

// ProjectToSurface (include/hpsdf.h): Newton's iteration onto {Query = iso} (project.hip, host_query.cpp)
int hpsdf_project_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dXyz, size_t n, double iso, double tol, uint32_t maxIter,
                         uint32_t flags, double* dOutXyz, double* dOutVal, double* dOutGrad, uint8_t* dOutIters, uint8_t* dOutStatus) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = projectArgumentError(flags, iso, tol, maxIter)) return rc;
    if (!t || (n && (!dXyz || !dOutXyz))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    TreeDev td;
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    HPSDF_HIP(launchProject(ctx->stream, td, ctx->dTables, dXyz, n, ProjectArgs{iso, tol, maxIter, flags}, dOutXyz, dOutVal, dOutGrad,
                            dOutIters, dOutStatus));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_project_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double iso, double tol, uint32_t maxIter,
                       uint32_t flags, double* outXyz, double* outVal, double* outGrad, uint8_t* outIters, uint8_t* outStatus) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = projectArgumentError(flags, iso, tol, maxIter)) return rc;
    if (!t || (n && (!xyz || !outXyz))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    if (n <= kHostQueryPoints && smallQueriesOnHost()) {
        if (const int hc = t->hostCopies()) return hc;
        hostProjectRows(*t, xyz, n, iso, tol, maxIter, flags, reductionLeftAssoc(ctx), outXyz, outVal, outGrad, outIters, outStatus);
        return HPSDF_OK;
    }
    // the input and the point output have device arrays of their own (outXyz may be xyz)
    HostArrays arr;
    const auto dXyz = arr.in(xyz, n * 3);
    const auto dOutXyz = arr.out(outXyz, n * 3);
    const auto dOutVal = arr.out(outVal, n);
    const auto dOutGrad = arr.out(outGrad, n * 3);
    const auto dOutIters = arr.out(outIters, n);
    const auto dOutStatus = arr.out(outStatus, n);
    return hostCall(ctx, arr, [&] {
        return hpsdf_project_device(ctx, t, dXyz, n, iso, tol, maxIter, flags, dOutXyz, dOutVal, dOutGrad, dOutIters, dOutStatus);
    });
    HPSDF_CATCH
}

// CastRays (include/hpsdf.h): the first crossing of each ray with {Query = iso} (cast_rays.hip, host_query.cpp)
int hpsdf_cast_rays_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dOrigins, const double* dDirs, const double* dTMax, size_t n,
                           double iso, double tol, uint32_t maxIter, uint32_t maxCells, uint32_t flags, uint8_t* dOutStatus, double* dOutT,
                           double* dOutXyz, double* dOutVal, double* dOutGrad, uint16_t* dOutEvals, uint16_t* dOutCells) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = castArgumentError(flags, iso, tol, maxIter, maxCells, n, dOrigins, dDirs, dTMax, dOutStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    TreeDev td;
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    HPSDF_HIP(launchCastRays(ctx->stream, td, ctx->dTables, dOrigins, dDirs, dTMax, n, CastArgs{iso, tol, maxIter, maxCells, flags, 0u},
                             dOutStatus, dOutT, dOutXyz, dOutVal, dOutGrad, dOutEvals, dOutCells));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_cast_rays_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* origins, const double* dirs, const double* tMax, size_t n, double iso,
                         double tol, uint32_t maxIter, uint32_t maxCells, uint32_t flags, uint8_t* outStatus, double* outT, double* outXyz,
                         double* outVal, double* outGrad, uint16_t* outEvals, uint16_t* outCells) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = castArgumentError(flags, iso, tol, maxIter, maxCells, n, origins, dirs, tMax, outStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    if (n <= kHostRays && smallQueriesOnHost()) {
        if (const int hc = t->hostCopies()) return hc;
        hostCastRows(*t, origins, dirs, tMax, n, CastArgs{iso, tol, maxIter, maxCells, flags, 0u}, reductionLeftAssoc(ctx), outStatus, outT, outXyz,
                     outVal, outGrad, outEvals, outCells);
        return HPSDF_OK;
    }
    HostArrays arr;
    const auto dOrigins = arr.in(origins, n * 3);
    const auto dDirs = arr.in(dirs, n * 3);
    const auto dTMax = arr.in(tMax, n);
    const auto dOutStatus = arr.out(outStatus, n);
    const auto dOutT = arr.out(outT, n);
    const auto dOutXyz = arr.out(outXyz, n * 3);
    const auto dOutVal = arr.out(outVal, n);
    const auto dOutGrad = arr.out(outGrad, n * 3);
    const auto dOutEvals = arr.out(outEvals, n);
    const auto dOutCells = arr.out(outCells, n);
    return hostCall(ctx, arr, [&] {
        return hpsdf_cast_rays_device(ctx, t, dOrigins, dDirs, dTMax, n, iso, tol, maxIter, maxCells, flags, dOutStatus, dOutT, dOutXyz, dOutVal,
                                      dOutGrad, dOutEvals, dOutCells);
    });
    HPSDF_CATCH
}

// QueryBounds (include/hpsdf.h): a guaranteed range of Query over boxes (query_bounds.hip, tree_bound.hpp, host_query.cpp).  The box and
// the grid entries differ in where a box comes from and in nothing else: boxes == nullptr means the cells of *grid.
static int boundsOnDevice(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dBoxes, const BoxGrid* grid, size_t n, uint32_t subdiv,
                          uint32_t maxLeaves, double* dOutLo, double* dOutHi, uint8_t* dOutStatus, uint32_t* dOutLeaves) {
    if (const int rc = treeOnContext(ctx, t)) return rc;
    if (const int rc = t->boundConsts(ctx)) return rc;  // (built by the first call on this tree; a load and a branch afterwards)
    HPSDF_HIP(launchQueryBounds(ctx->stream, clsTreeOnDevice(t), t->maxDegree, ctx->dTables, dBoxes, grid, n, subdiv, maxLeaves, dOutLo, dOutHi,
                                dOutStatus, dOutLeaves));
    return HPSDF_OK;
}

static int boundsOnHost(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* boxes, const BoxGrid* grid, size_t n, uint32_t subdiv, uint32_t maxLeaves,
                        double* outLo, double* outHi, uint8_t* outStatus, uint32_t* outLeaves) {
    if (n <= kHostQueryPoints && smallQueriesOnHost()) {
        if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
        if (const int hc = t->hostCopies()) return hc;
        if (const int hc = t->boundHostCopies(ctx)) return hc;
        hostBoundsRows(clsTreeOnHost(t), boxes, grid, n, subdiv, maxLeaves, outLo, outHi, outStatus, outLeaves);
        return HPSDF_OK;
    }
    HostArrays arr;
    const HostArrays::Dev<const double> dBoxes = boxes ? arr.in(boxes, n * 6) : HostArrays::Dev<const double>{nullptr};
    const auto dOutLo = arr.out(outLo, n);
    const auto dOutHi = arr.out(outHi, n);
    const auto dOutStatus = arr.out(outStatus, n);
    const auto dOutLeaves = arr.out(outLeaves, n);
    return hostCall(ctx, arr, [&] { return boundsOnDevice(ctx, t, dBoxes, grid, n, subdiv, maxLeaves, dOutLo, dOutHi, dOutStatus, dOutLeaves); });
}

int hpsdf_query_bounds_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dBoxes, size_t n, uint32_t subdiv, uint32_t maxLeaves,
                              double* dOutLo, double* dOutHi, uint8_t* dOutStatus, uint32_t* dOutLeaves) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = boundsArgumentError(subdiv, maxLeaves, n, dBoxes, dOutLo, dOutHi, dOutStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    return boundsOnDevice(ctx, t, dBoxes, nullptr, n, subdiv, maxLeaves, dOutLo, dOutHi, dOutStatus, dOutLeaves);
    HPSDF_CATCH
}

int hpsdf_query_bounds_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* boxes, size_t n, uint32_t subdiv, uint32_t maxLeaves, double* outLo,
                            double* outHi, uint8_t* outStatus, uint32_t* outLeaves) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = boundsArgumentError(subdiv, maxLeaves, n, boxes, outLo, outHi, outStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (n == 0) return HPSDF_OK;
    return boundsOnHost(ctx, t, boxes, nullptr, n, subdiv, maxLeaves, outLo, outHi, outStatus, outLeaves);
    HPSDF_CATCH
}

int hpsdf_query_bounds_grid_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3],
                                   uint32_t subdiv, uint32_t maxLeaves, double* dOutLo, double* dOutHi, uint8_t* dOutStatus,
                                   uint32_t* dOutLeaves) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!lo || !hi || !n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = boundsArgumentError(subdiv, maxLeaves, 1, lo, dOutLo, dOutHi, dOutStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    BoxGrid g{};
    size_t count = 0;
    if (const int rc = checkBoundsGrid("hpsdf_query_bounds_grid_device", t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, &g, &count)) return rc;
    return boundsOnDevice(ctx, t, nullptr, &g, count, subdiv, maxLeaves, dOutLo, dOutHi, dOutStatus, dOutLeaves);
    HPSDF_CATCH
}

int hpsdf_query_bounds_grid_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3], uint32_t subdiv,
                                 uint32_t maxLeaves, double* outLo, double* outHi, uint8_t* outStatus, uint32_t* outLeaves) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!lo || !hi || !n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = boundsArgumentError(subdiv, maxLeaves, 1, lo, outLo, outHi, outStatus)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    BoxGrid g{};
    size_t count = 0;
    if (const int rc = checkBoundsGrid("hpsdf_query_bounds_grid_host", t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, &g, &count)) return rc;
    return boundsOnHost(ctx, t, nullptr, &g, count, subdiv, maxLeaves, outLo, outHi, outStatus, outLeaves);
    HPSDF_CATCH
}

// Integrate (include/hpsdf.h): volume bounds and moments of the solid (integrate.hip, integrate.hpp, host_query.cpp)
int hpsdf_integrate_device(hpsdf_ctx* ctx, const hpsdf_tree* t, double iso, uint32_t depth, uint32_t samples, uint32_t maxCells, hpsdf_integral* out,
                           hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = integrateArgumentError(iso, depth, samples, maxCells, out, outCells, outCount)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (const int rc = treeOnContext(ctx, t)) return rc;
    if (const int rc = t->boundConsts(ctx)) return rc;
    if (const int rc = t->integrateLeaves(ctx)) return rc;
    const IntegrateArgs a{iso, depth, samples, maxCells};
    return integrateOnDevice(ctx, clsTreeOnDevice(t), t->maxDegree, t->dLeafCells, t->nLeafCells, a, out, outCells, outCount);
    HPSDF_CATCH
}

int hpsdf_integrate_host(hpsdf_ctx* ctx, const hpsdf_tree* t, double iso, uint32_t depth, uint32_t samples, uint32_t maxCells, hpsdf_integral* out,
                         hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = integrateArgumentError(iso, depth, samples, maxCells, out, outCells, outCount)) return rc;
    if (!t) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    if (const int hc = t->hostCopies()) return hc;
    if (const int hc = t->boundHostCopies(ctx)) return hc;
    const IntegrateArgs a{iso, depth, samples, maxCells};
    return hostIntegrate(clsTreeOnHost(t), t->hRecs.size(), a, out, outCells, outCount);
    HPSDF_CATCH
}

// IntegratePair (include/hpsdf.h): Integrate over A with every cell also classified against B under a pose (integrate_pair.hip,
// integrate_pair.hpp, integrate_pair_host.cpp)
int hpsdf_integrate_pair_device(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, uint32_t op, const double pose[12], double isoA,
                                double isoB, uint32_t depth, uint32_t samples, uint32_t maxCells, uint32_t maxLeaves, hpsdf_integral* out,
                                hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = pairArgumentError(op, pose, isoA, isoB, depth, samples, maxCells, maxLeaves, out, outCells, outCount)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: the two trees live on different devices");
    if (const int rc = treeOnContext(ctx, tA)) return rc;
    if (const int rc = tA->boundConsts(ctx)) return rc;
    if (const int rc = tB->boundConsts(ctx)) return rc;
    if (const int rc = tA->integrateLeaves(ctx)) return rc;
    const ClsTree ctA = clsTreeOnDevice(tA), ctB = clsTreeOnDevice(tB);
    const PairArgs p = pairArgs(ctA, op, pose, isoA, isoB, maxLeaves);
    const IntegrateArgs a{isoA, depth, samples, maxCells};
    return integratePairOnDevice(ctx, ctA, ctB, std::max(tA->maxDegree, tB->maxDegree), tA->dLeafCells, tA->nLeafCells, p, a, out, outCells, outCount);
    HPSDF_CATCH
}

int hpsdf_integrate_pair_host(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, uint32_t op, const double pose[12], double isoA,
                              double isoB, uint32_t depth, uint32_t samples, uint32_t maxCells, uint32_t maxLeaves, hpsdf_integral* out,
                              hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = pairArgumentError(op, pose, isoA, isoB, depth, samples, maxCells, maxLeaves, out, outCells, outCount)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: the two trees live on different devices");
    if (tA->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    for (const hpsdf_tree* t : {tA, tB}) {
        if (const int hc = t->hostCopies()) return hc;
        if (const int hc = t->boundHostCopies(ctx)) return hc;
    }
    const ClsTree ctA = clsTreeOnHost(tA), ctB = clsTreeOnHost(tB);
    const PairArgs p = pairArgs(ctA, op, pose, isoA, isoB, maxLeaves);
    const IntegrateArgs a{isoA, depth, samples, maxCells};
    return hostIntegratePair(ctA, tA->hRecs.size(), ctB, p, a, out, outCells, outCount);
    HPSDF_CATCH
}

// Clearance (include/hpsdf.h): the guaranteed minimum of B's field over A's solid under a pose (clearance.hip, clearance.hpp,
// clearance_host.cpp)
int hpsdf_clearance_device(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, const double pose[12], double isoA, uint32_t depth, double tol,
                           uint32_t maxCells, uint32_t maxLeaves, hpsdf_clearance* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = clearanceArgumentError(pose, isoA, depth, tol, maxCells, maxLeaves, out, outCells, outCount)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: the two trees live on different devices");
    if (const int rc = treeOnContext(ctx, tA)) return rc;
    if (const int rc = tA->boundConsts(ctx)) return rc;
    if (const int rc = tB->boundConsts(ctx)) return rc;
    if (const int rc = tA->integrateLeaves(ctx)) return rc;
    const ClsTree ctA = clsTreeOnDevice(tA), ctB = clsTreeOnDevice(tB);
    const PairArgs p = pairArgs(ctA, HPSDF_PAIR_INTERSECTION, pose, isoA, 0.0, maxLeaves);
    const ClearanceArgs a{depth, maxCells, tol};
    return clearanceOnDevice(ctx, ctA, ctB, std::max(tA->maxDegree, tB->maxDegree), tA->dLeafCells, tA->nLeafCells, p, a, out, outCells, outCount);
    HPSDF_CATCH
}

int hpsdf_clearance_host(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, const double pose[12], double isoA, uint32_t depth, double tol,
                         uint32_t maxCells, uint32_t maxLeaves, hpsdf_clearance* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = clearanceArgumentError(pose, isoA, depth, tol, maxCells, maxLeaves, out, outCells, outCount)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: the two trees live on different devices");
    if (tA->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    for (const hpsdf_tree* t : {tA, tB}) {
        if (const int hc = t->hostCopies()) return hc;
        if (const int hc = t->boundHostCopies(ctx)) return hc;
    }
    const ClsTree ctA = clsTreeOnHost(tA), ctB = clsTreeOnHost(tB);
    const PairArgs p = pairArgs(ctA, HPSDF_PAIR_INTERSECTION, pose, isoA, 0.0, maxLeaves);
    const ClearanceArgs a{depth, maxCells, tol};
    return hostClearance(ctA, tA->hRecs.size(), ctB, p, a, out, outCells, outCount);
    HPSDF_CATCH
}

// ClearanceBatch (include/hpsdf.h, "Clearance", "Batches"): Clearance for n poses in one call (clearance_batch.hip; the host entry is a
// loop of hostClearance)
int hpsdf_clearance_batch_device(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, const double* poses, size_t n, double isoA, uint32_t depth,
                                 double tol, double decide, uint32_t maxCells, uint32_t maxLeaves, uint32_t maxTotalCells, hpsdf_clearance* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (n == 0) return HPSDF_OK;
    if (const int rc = clearanceBatchArgumentError(poses, n, isoA, depth, tol, decide, maxCells, maxLeaves, maxTotalCells, out)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: the two trees live on different devices");
    if (const int rc = treeOnContext(ctx, tA)) return rc;
    if (const int rc = tA->boundConsts(ctx)) return rc;
    if (const int rc = tB->boundConsts(ctx)) return rc;
    if (const int rc = tA->integrateLeaves(ctx)) return rc;
    const ClearanceArgs a{depth, maxCells, tol, decide};
    return clearanceBatchOnDevice(ctx, clsTreeOnDevice(tA), clsTreeOnDevice(tB), std::max(tA->maxDegree, tB->maxDegree), tA->dLeafCells, tA->nLeafCells,
                                  poses, n, isoA, maxLeaves, a, maxTotalCells, out);
    HPSDF_CATCH
}

int hpsdf_clearance_batch_host(hpsdf_ctx* ctx, const hpsdf_tree* tA, const hpsdf_tree* tB, const double* poses, size_t n, double isoA, uint32_t depth,
                               double tol, double decide, uint32_t maxCells, uint32_t maxLeaves, uint32_t maxTotalCells, hpsdf_clearance* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (n == 0) return HPSDF_OK;
    if (const int rc = clearanceBatchArgumentError(poses, n, isoA, depth, tol, decide, maxCells, maxLeaves, maxTotalCells, out)) return rc;
    if (!tA || !tB) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null tree");
    if (tA->device != tB->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: the two trees live on different devices");
    if (tA->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    for (const hpsdf_tree* t : {tA, tB}) {
        if (const int hc = t->hostCopies()) return hc;
        if (const int hc = t->boundHostCopies(ctx)) return hc;
    }
    const ClearanceArgs a{depth, maxCells, tol, decide};
    return hostClearanceBatch(clsTreeOnHost(tA), tA->hRecs.size(), clsTreeOnHost(tB), poses, n, isoA, maxLeaves, a, out);
    HPSDF_CATCH
}

// Simplify (include/hpsdf.h): a coarser tree from a serialised one, within an RMS bound (simplify.hip, simplify.hpp; the device-free
// entry is simplify_host.cpp's)
int hpsdf_simplify(hpsdf_ctx* ctx, const void* block, size_t size, double rms, uint32_t flags, void** out_block, size_t* out_size,
                   hpsdf_simplify_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = simplifyArgumentError(rms, flags, out_block, out_size)) return rc;
    const Tables& T = tables();
    BlockView v;
    BlockMirror m;
    std::string why;
    int rc = readBlock(block, size, v, why);
    if (!rc) rc = mirrorBlock(v, T, m, why);
    if (rc) return fail(rc, why);
    HPSDF_HIP(hipSetDevice(ctx->device));
    SimpState s;
    simplifyBegin(v, m, T, s);
    if (const int drc = simplifyOnDevice(ctx, v, m, rms, flags, s)) return drc;
    rc = simplifyAssemble(v, T, s, [ctx](size_t n) { return ctx->allocBlock(n); }, out_block, out_size, stats, why);
    return rc ? fail(rc, why) : HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_surface_project_vertices(hpsdf_ctx* ctx, const hpsdf_tree* t, double* verts, uint64_t nv, const double h[3], double iso,
                                   double tol, uint32_t maxIter, uint64_t* nMoved) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (const int rc = projectArgumentError(0u, iso, tol, maxIter)) return rc;
    if (!t || (nv && !verts) || !h) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    for (int a = 0; a < 3; ++a)
        if (!(h[a] >= 0.0)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_surface_project_vertices: h must be >= 0 on every axis");
    if (nMoved) *nMoved = 0;
    if (nv == 0) return HPSDF_OK;
    std::vector<double> moved(3 * (size_t)nv);
    std::vector<uint8_t> status((size_t)nv);
    if (const int rc = hpsdf_project_host(ctx, t, verts, (size_t)nv, iso, tol, maxIter, 0u, moved.data(), nullptr, nullptr, nullptr, status.data()))
        return rc;
    uint64_t count = 0;
    for (size_t i = 0; i < (size_t)nv; ++i) {
        const double* m = &moved[3 * i];
        double* v = verts + 3 * i;
        // a converged projection that stays within half a cube of the vertex on every axis; anything else leaves the vertex as it was
        if (status[i] == HPSDF_PROJECT_CONVERGED && std::fabs(m[0] - v[0]) <= 0.5 * h[0] && std::fabs(m[1] - v[1]) <= 0.5 * h[1] &&
            std::fabs(m[2] - v[2]) <= 0.5 * h[2]) {
            v[0] = m[0], v[1] = m[1], v[2] = m[2];
            ++count;
        }
    }
    if (nMoved) *nMoved = count;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_query_ray_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* dOrigins, const double* dDirs,
                           const double* dTMax, size_t n, uint8_t* dHit, double* dT) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (n && (!dOrigins || !dDirs || !dTMax || !dHit || !dT))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    TreeDev td;  // (query_ray_kernel reads no reduction order)
    if (const int rc = treeOnContext(ctx, t, &td)) return rc;
    HPSDF_HIP(launchQueryRay(ctx->stream, td, ctx->dTables, dOrigins, dDirs, dTMax, n, dHit, dT));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_query_ray_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* origins, const double* dirs,
                         const double* tMax, size_t n, uint8_t* hit, double* tOut) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || (n && (!origins || !dirs || !tMax || !hit || !tOut))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    if (n <= hostRayLimit() && smallQueriesOnHost()) {  // a scalar QueryRay(ray, tMax, t): <= 200 host Query steps instead of a launch
        if (const int hc = t->hostCopies()) return hc;
        for (size_t i = 0; i < n; ++i) hit[i] = hostQueryRay(*t, origins + 3 * i, dirs + 3 * i, tMax[i], tOut + i) ? 1 : 0;
        return HPSDF_OK;
    }
    // t of a miss keeps the caller's value (the reference leaves t_ untouched)
    HostArrays arr;
    const auto dOrigins = arr.in(origins, n * 3);
    const auto dDirs = arr.in(dirs, n * 3);
    const auto dTMax = arr.in(tMax, n);
    const auto dT = arr.inout(tOut, n);
    const auto dHit = arr.out(hit, n);
    return hostCall(ctx, arr, [&] { return hpsdf_query_ray_device(ctx, t, dOrigins, dDirs, dTMax, n, dHit, dT); });
    HPSDF_CATCH
}

// (u8)f64 as the reference's x86-64 build performs it: truncating conversion to a 32-bit integer
// (out of range and NaN give INT_MIN), then the low byte
static uint8_t f64ToU8(double q) {
    int32_t v;
    if (!(q > -2147483649.0 && q < 2147483648.0))
        v = INT32_MIN;
    else
        v = (int32_t)q;
    return (uint8_t)(v & 0xFF);
}

int hpsdf_function_slice(hpsdf_ctx* ctx, const hpsdf_tree* t, double c, const float* viewMin, const float* viewMax,
                         uint64_t nSamples, uint8_t* rgb, double* values) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || !viewMin || !viewMax || !rgb) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (nSamples == 0 || nSamples > 32768) return fail(HPSDF_ERR_INVALID_ARGUMENT, "n_samples must be in [1, 32768]");
    if (const int rc = treeOnContext(ctx, t)) return rc;
    const size_t total = (size_t)nSamples * nSamples;
    DevBufs bufs;
    double *dV = nullptr, *dP = nullptr;
    HPSDF_HIP(bufs.alloc((void**)&dV, total * sizeof(double)));
    HPSDF_HIP(bufs.alloc((void**)&dP, total * 3 * sizeof(double)));
    const float step = (viewMax[0] - viewMin[0]) / (float)nSamples;  // Octree.cpp:1149
    HPSDF_HIP(launchSlicePoints(ctx->stream, c, viewMin[0], viewMin[1], step, (uint32_t)nSamples, dP));
    {
        const int rc = queryDevice(ctx, t, dP, total, dV, nullptr);
        if (rc) return rc;
    }
    std::vector<double> own;
    double* v = values;
    if (!v) {
        own.resize(total);
        v = own.data();
    }
    HPSDF_HIP(hipMemcpyAsync(v, dV, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HPSDF_HIP(hipStreamSynchronize(ctx->stream));
    // Octree.cpp:1140-1167 ranges, :1172-1196 bytes
    double posFirst = DBL_MAX, posSecond = 0.0, negFirst = 0.0, negSecond = DBL_MAX * -1.0;
    for (size_t p = 0; p < total; ++p) {
        const double s = v[p];
        if (s > (double)0.000001f) {
            posFirst = std::min(s, posFirst);
            posSecond = std::max(s, posSecond);
        } else {
            negFirst = std::min(s, negFirst);
            negSecond = std::max(s, negSecond);
        }
    }
    for (size_t p = 0; p < total; ++p) {
        const float u = (float)v[p];
        uint8_t* px = rgb + 3 * p;
        if (u > 0.0f) {
            px[0] = 0, px[1] = f64ToU8(255 * ((double)u - posSecond) / (posFirst - posSecond)), px[2] = 0;
        } else {
            px[0] = 0, px[1] = 0, px[2] = f64ToU8(255 * ((double)u - negFirst) / (negSecond - negFirst));
        }
    }
    return HPSDF_OK;
    HPSDF_CATCH
}

}  // extern "C"
