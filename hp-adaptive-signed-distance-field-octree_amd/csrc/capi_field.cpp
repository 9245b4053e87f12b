// C ABI of include/hpsdf.h: the four kinds of field, a mesh field's host mirror and the field evaluation entries.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>

#include "frontier_dev.hpp"
#include "host_call.hpp"
#include "launch.hpp"
#include "runtime.hpp"

using namespace hpsdf;

namespace hpsdf {
int loadObj(const char* path, std::vector<float>& verts, std::vector<uint64_t>& tris, std::string& err);  // obj.cpp
}

extern "C" {

// ---------------------------------------------------------------------------- fields
int hpsdf_field_create_analytic(const hpsdf_prim* prims, int n, hpsdf_field** out) {
    HPSDF_TRY
    if (!prims || !out || n < 1 || n > HPSDF_MAX_PRIMS)
        return fail(HPSDF_ERR_INVALID_ARGUMENT, "analytic field needs 1..HPSDF_MAX_PRIMS primitives");
    for (int i = 0; i < n; ++i)
        if (prims[i].kind < 0 || prims[i].kind > HPSDF_PRIM_PLANE || prims[i].op < 0 || prims[i].op > HPSDF_OP_SUBTRACT)
            return fail(HPSDF_ERR_INVALID_ARGUMENT, "unknown primitive kind or op");
    hpsdf_field* f = new hpsdf_field();
    f->kind = kHostAnalytic;
    f->prims.assign(prims, prims + n);
    *out = f;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_create_callback(hpsdf_callback cb, void* user, hpsdf_field** out) {
    HPSDF_TRY
    if (!cb || !out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null callback");
    hpsdf_field* f = new hpsdf_field();
    f->kind = kHostCallback;
    f->cb = cb;
    f->user = user;
    *out = f;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_create_mesh(hpsdf_ctx* ctx, const float* verts, uint64_t nVerts, const uint64_t* tris, uint64_t nTris,
                            hpsdf_field** out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "mesh fields live in HBM: a device context is required");
    if (!verts || !tris || !out || nVerts == 0 || nTris == 0) return fail(HPSDF_ERR_INVALID_ARGUMENT, "empty mesh");
    if (nVerts > 0x7FFFFFFFull || nTris > kMeshMaxTris) return fail(HPSDF_ERR_UNSUPPORTED, "mesh too large: at most 2^27 - 1 triangles");
    HPSDF_HIP(hipSetDevice(ctx->device));
    hpsdf_field* f = new hpsdf_field();
    f->kind = kHostMesh;
    f->device = ctx->device;
    hipError_t e = hipSuccess;
    // half-edge twins and BVH on the device (mesh_build.hip); HPSDF_MESH_HOST_BUILD=1, non-manifold input and single
    // triangles take the host preparation of mesh.cpp (same field values either way: any BVH gives the same distances)
    int fallback = 1;
    {
        const char* hb = std::getenv("HPSDF_MESH_HOST_BUILD");
        if (!(hb && hb[0] == '1')) {
            const int brc = meshBuildDevice(ctx, verts, nVerts, tris, nTris, f, &fallback);
            if (brc != HPSDF_OK) {
                delete f;
                return brc;
            }
        }
    }
    if (fallback == 2) {  // non-manifold: the twins from the host's sequential pairing, everything else is on the device already
        std::vector<uint32_t> he;
        if (!hostHalfEdges(tris, nTris, nVerts, &he)) {
            hpsdf_field_destroy(f);
            return fail(HPSDF_ERR_OPEN_MESH, "mesh is not closed: an edge has no twin (Mesh::CreateHalfEdges)");
        }
        e = hipMemcpy(f->dHalfEdges, he.data(), he.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    } else if (fallback) {
        for (uint64_t i = 0; i < 3 * nTris; ++i)
            if (tris[i] >= nVerts) {
                delete f;
                return fail(HPSDF_ERR_INVALID_ARGUMENT, "triangle " + std::to_string(i / 3) + " refers to vertex " + std::to_string(tris[i]) +
                                                            " of " + std::to_string(nVerts));
            }
        HostMesh hm;
        if (!prepareMesh(verts, nVerts, tris, nTris, &hm)) {
            delete f;
            return fail(HPSDF_ERR_OPEN_MESH, "mesh is not closed: an edge has no twin (Mesh::CreateHalfEdges)");
        }
        f->nVerts = (uint32_t)nVerts;
        f->nTris = (uint32_t)nTris;
        f->nBvhNodes = (uint32_t)hm.bvh.size();
        auto up = [&](void** d, const void* h, size_t bytes) -> hipError_t {
            hipError_t ue = hipMalloc(d, bytes);
            if (ue != hipSuccess) return ue;
            return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
        };
        e = up((void**)&f->dVerts, hm.verts.data(), hm.verts.size() * sizeof(float));
        if (e == hipSuccess) e = up((void**)&f->dTris, hm.tris.data(), hm.tris.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&f->dTriPos, (size_t)nTris * kTriRecordFloats * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&f->dTriPre, (size_t)nTris * kTriPreFloats * sizeof(float));
        if (e == hipSuccess) e = launchMeshTriPos(ctx->stream, f->dVerts, f->dTris, nTris, f->dTriPos, nullptr, f->dTriPre);  // after the blocking uploads
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = up((void**)&f->dHalfEdges, hm.halfEdges.data(), hm.halfEdges.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = up((void**)&f->dBvh, hm.bvh.data(), hm.bvh.size() * sizeof(BvhNode));
    }
#ifdef HPSDF_MESH_STATS_BUILD
    if (e == hipSuccess && std::getenv("HPSDF_MESH_STATS")) {
        e = hipMalloc((void**)&f->dStats, 8 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(f->dStats, 0, 8 * sizeof(unsigned long long));
    }
#endif
    if (e != hipSuccess) {
        hpsdf_field_destroy(f);
        return hipFail(e, "mesh upload");
    }
    *out = f;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_obj_load(const char* path, float** verts, uint64_t* nVerts, uint64_t** tris, uint64_t* nTris) {
    HPSDF_TRY
    if (!path || !verts || !nVerts || !tris || !nTris) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *verts = nullptr, *tris = nullptr, *nVerts = 0, *nTris = 0;
    std::vector<float> v;
    std::vector<uint64_t> t;
    std::string err;
    const int rc = loadObj(path, v, t, err);
    if (rc) return fail(rc, err);
    *verts = (float*)std::malloc(v.size() * sizeof(float));
    *tris = (uint64_t*)std::malloc(t.size() * sizeof(uint64_t));
    if (!*verts || !*tris) {
        std::free(*verts), std::free(*tris);
        *verts = nullptr, *tris = nullptr;
        return fail(HPSDF_ERR_OUT_OF_MEMORY, "malloc failed");
    }
    std::memcpy(*verts, v.data(), v.size() * sizeof(float));
    std::memcpy(*tris, t.data(), t.size() * sizeof(uint64_t));
    *nVerts = v.size() / 3;
    *nTris = t.size() / 3;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_create_tree_csg(const hpsdf_tree* old, int op, const hpsdf_field* inner, hpsdf_field** out) {
    HPSDF_TRY
    if (!old || !inner || !out || op < 0 || op > HPSDF_OP_SUBTRACT)
        return fail(HPSDF_ERR_INVALID_ARGUMENT, "bad csg field arguments");
    if (inner->kind == kHostTreeCsg) return fail(HPSDF_ERR_UNSUPPORTED, "nested csg fields are not supported");
    hpsdf_field* f = new hpsdf_field();
    f->kind = kHostTreeCsg;
    f->oldTree = old;
    f->csgOp = op;
    f->inner = inner;
    *out = f;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_destroy(hpsdf_field* f) {
    if (!f) return HPSDF_OK;
    if (f->kind == kHostMesh && f->device >= 0) {
        (void)hipSetDevice(f->device);
        if (f->dBlock) {
            (void)hipFree(f->dBlock);
            hpsdf::meshPoolTrim(f->device);
        } else {
            if (f->dVerts) (void)hipFree(f->dVerts);
            if (f->dTris) (void)hipFree(f->dTris);
            if (f->dTriPos) (void)hipFree(f->dTriPos);
            if (f->dTriPre) (void)hipFree(f->dTriPre);
            if (f->dHalfEdges) (void)hipFree(f->dHalfEdges);
            if (f->dBvh) (void)hipFree(f->dBvh);
        }
        if (f->dStats) (void)hipFree(f->dStats);
    }
    delete f;
    return HPSDF_OK;
}

int hpsdf_field_mesh_stats(const hpsdf_field* f, uint64_t out[8], int reset) {
    HPSDF_TRY
    if (!f || !out || f->kind != kHostMesh) return fail(HPSDF_ERR_INVALID_ARGUMENT, "not a mesh field");
    if (!f->dStats) return fail(HPSDF_ERR_UNSUPPORTED, "traversal counters need a diagnostic build (-DHPSDF_MESH_STATS_BUILD) and HPSDF_MESH_STATS=1");
    HPSDF_HIP(hipSetDevice(f->device));
    HPSDF_HIP(hipDeviceSynchronize());
    HPSDF_HIP(hipMemcpy(out, f->dStats, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HPSDF_HIP(hipMemset(f->dStats, 0, 8 * sizeof(uint64_t)));
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_eval_device(hpsdf_ctx* ctx, const hpsdf_field* f, const double* dXyz, size_t n, double* dOut) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!f || (!dXyz && n) || (!dOut && n)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (innermost(f)->kind == kHostCallback) return fail(HPSDF_ERR_UNSUPPORTED, "callback fields are evaluated on the host");
    HPSDF_HIP(hipSetDevice(ctx->device));
    FieldDev fd;
    int rc = makeFieldDev(ctx, f, nullptr, &fd);
    if (rc) return rc;
    // A plain mesh field goes through the sampler's traversal, 64 consecutive points per walk (meshSignedDistanceWaveQ:
    // dense nodes walked by the wave, sparse subtrees pooled, tests compacted) -- the same bits as the per-point traversal
    // and 4 (random points) to 8 (points sorted by cell) times its speed on a 2 M-triangle mesh.
    // (Not under hpsdf_set_mesh_face_rule(1): the shared traversal's bounds -- slabs, in-plane rectangles -- bound the DISTANCE to a
    // triangle, and the reference's face-case point can lie below it; the per-point traversal prunes by boxes alone, as the reference's does.)
    if (fd.kind == kFieldMesh && fd.csgOp < 0 && !meshFaceRuleReference(ctx))
        HPSDF_HIP(launchMeshEvalWave(ctx->stream, fd, dXyz, n, dOut));
    else
        HPSDF_HIP(launchFieldEval(ctx->stream, fd, ctx->dTables, dXyz, n, dOut));
    return HPSDF_OK;
    HPSDF_CATCH
}

// What the host copies of a mesh field's arrays weigh, and up to where they are made at all: beyond HPSDF_HOST_MESH_MIRROR_MB (default
// 512) a call of a few points is a launch like any other -- a mirror of a 2 M-triangle mesh is ~330 MB of pageable memory, fetched
// behind a device-wide synchronisation (the field's arrays may still be being written on some stream), under the field's lock, and kept
// until hpsdf_field_release_host_copies() or the field's destruction.
static size_t meshMirrorBytes(const hpsdf_field* f) {
    return (size_t)f->nVerts * 12 + (size_t)f->nTris * (12 + 12 + 4 * (size_t)(kTriRecordFloats + kTriPreFloats)) + (size_t)f->nBvhNodes * sizeof(BvhNode);
}
static size_t hostMeshMirrorLimit() { static const size_t v = hostLimit("HPSDF_HOST_MESH_MIRROR_MB", 512) << 20; return v; }
// Where the host copies of a mesh field's device arrays go: the ONE list of what a mesh field holds on the device, for the mirror below
// and for hpsdf_field_mesh_arrays.  A null destination is skipped; slabs exist on device-built fields only.  Reads the device, writes the host.
struct MeshArraysDst {
    float* verts = nullptr;
    uint32_t* tris = nullptr;
    float* triPos = nullptr;
    float* triPre = nullptr;
    uint32_t* halfEdges = nullptr;
    BvhNode* bvh = nullptr;
    NodeSlab* slabs = nullptr;
};
constexpr int kMeshArrays = 7;
static void meshArrayBytes(const hpsdf_field* f, size_t bytes[kMeshArrays]) {
    bytes[0] = 3 * (size_t)f->nVerts * sizeof(float), bytes[1] = 3 * (size_t)f->nTris * sizeof(uint32_t);
    bytes[2] = (size_t)kTriRecordFloats * f->nTris * sizeof(float), bytes[3] = (size_t)kTriPreFloats * f->nTris * sizeof(float);
    bytes[4] = 3 * (size_t)f->nTris * sizeof(uint32_t), bytes[5] = (size_t)f->nBvhNodes * sizeof(BvhNode);
    bytes[6] = f->dSlabs ? (size_t)f->nBvhNodes * sizeof(NodeSlab) : 0;
}
static int meshDownload(const hpsdf_field* f, const MeshArraysDst& d) {
    size_t bytes[kMeshArrays];
    meshArrayBytes(f, bytes);
    void* const dst[kMeshArrays] = {d.verts, d.tris, d.triPos, d.triPre, d.halfEdges, d.bvh, d.slabs};
    const void* const src[kMeshArrays] = {f->dVerts, f->dTris, f->dTriPos, f->dTriPre, f->dHalfEdges, f->dBvh, f->dSlabs};
    HPSDF_HIP(hipSetDevice(f->device));
    HPSDF_HIP(hipDeviceSynchronize());  // (the field's arrays may still be being written on some stream)
    for (int i = 0; i < kMeshArrays; ++i)
        if (dst[i] && src[i] && bytes[i]) HPSDF_HIP(hipMemcpy(dst[i], src[i], bytes[i], hipMemcpyDeviceToHost));
    return HPSDF_OK;
}
// The host copies of a mesh field's arrays (made once, by the first call of a few points)
static int meshHostMirror(const hpsdf_field* f, std::shared_ptr<hpsdf_field::HostMirror>* out) {
    std::lock_guard<std::mutex> guard(f->hostMirrorLock);
    if (!f->hostMirror) {
        auto m = std::make_shared<hpsdf_field::HostMirror>();
        m->verts.resize(3 * (size_t)f->nVerts);
        m->tris.resize(3 * (size_t)f->nTris);
        m->halfEdges.resize(3 * (size_t)f->nTris);
        m->triPos.resize((size_t)kTriRecordFloats * f->nTris);
        m->triPre.resize((size_t)kTriPreFloats * f->nTris);
        m->bvh.resize(std::max<size_t>(1, f->nBvhNodes));
        MeshArraysDst dst;
        dst.verts = m->verts.data(), dst.tris = m->tris.data(), dst.triPos = m->triPos.data(), dst.triPre = m->triPre.data();
        dst.halfEdges = m->halfEdges.data(), dst.bvh = m->bvh.data();  // (no slabs: the per-point traversal uses boxes and triangle records only)
        const int rc = meshDownload(f, dst);
        if (rc) return rc;
        MeshDev& d = m->dev;
        d.verts = m->verts.data(), d.tris = m->tris.data(), d.halfEdges = m->halfEdges.data();
        d.triPos = reinterpret_cast<const float4*>(m->triPos.data());
        d.triPre = reinterpret_cast<const float4*>(m->triPre.data());
        d.bvh = m->bvh.data(), d.slabs = nullptr;
        d.nTris = f->nTris, d.nNodes = f->nBvhNodes, d.leafLog2 = f->leafLog2, d.poolCap = 0, d.stats = nullptr;
        f->hostMirror = m;
    }
    *out = f->hostMirror;
    return HPSDF_OK;
}

int hpsdf_field_mesh_arrays(const hpsdf_field* f, uint64_t info[5], void* const* buffers, const uint64_t* capacities) {
    HPSDF_TRY
    if (!f || !info || f->kind != kHostMesh || f->device < 0) return fail(HPSDF_ERR_INVALID_ARGUMENT, "not a mesh field");
    if (buffers && !capacities) return fail(HPSDF_ERR_INVALID_ARGUMENT, "buffers without their capacities");
    size_t bytes[kMeshArrays];
    meshArrayBytes(f, bytes);
    if (buffers) {
        for (int i = 0; i < kMeshArrays; ++i)
            if (buffers[i] && capacities[i] < bytes[i])
                return fail(HPSDF_ERR_INVALID_ARGUMENT, "mesh array " + std::to_string(i) + " needs " + std::to_string(bytes[i]) + " bytes");
        MeshArraysDst dst;
        dst.verts = (float*)buffers[0], dst.tris = (uint32_t*)buffers[1], dst.triPos = (float*)buffers[2], dst.triPre = (float*)buffers[3];
        dst.halfEdges = (uint32_t*)buffers[4], dst.bvh = (BvhNode*)buffers[5], dst.slabs = (NodeSlab*)buffers[6];
        const int rc = meshDownload(f, dst);
        if (rc) return rc;
    }
    info[0] = f->nVerts, info[1] = f->nTris, info[2] = f->nBvhNodes, info[3] = f->leafLog2, info[4] = f->dSlabs ? 1 : 0;
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_field_release_host_copies(hpsdf_field* f) {
    if (!f) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null field");
    std::lock_guard<std::mutex> guard(f->hostMirrorLock);
    f->hostMirror.reset();  // (calls in flight hold their own reference)
    return HPSDF_OK;
}

int hpsdf_field_eval_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!f || (!xyz && n) || (!out && n)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    // Mesh::SignedDistanceAtPt(pt, bvh): a call of a few points on a plain mesh field never reaches the device (~57 us as a launch;
    // a user's SDF lambda that calls it per sample -- the reference's own usage, Mesh.cpp:54-63 -- would cost minutes per Create)
    if (n && n <= hostMeshLimit() && f->kind == kHostMesh && f->nTris >= 1 && f->nBvhNodes >= 1 && smallQueriesOnHost() &&
        meshMirrorBytes(f) <= hostMeshMirrorLimit()) {
        std::shared_ptr<hpsdf_field::HostMirror> m;
        const int rc = meshHostMirror(f, &m);
        if (rc) return rc;
        MeshDev hm = m->dev;
        hm.faceTolOfSlack = meshFaceTolOfSlack(ctx);  // (the rule at the time of the call, as on the device)
        meshEvalHostPoints(hm, xyz, n, out);
        return HPSDF_OK;
    }
    return hostRoundTrip(ctx, xyz, n, out, [&](const double* d, double* r) { return hpsdf_field_eval_device(ctx, f, d, n, r); });
    HPSDF_CATCH
}

// A mesh field's distance by one of its three diagnostic paths: the linear scan, the sampler's shared traversal, and the per-point stack
// traversal (what a mesh field wrapped by a tree-CSG and the fused mesh fit run)
enum MeshDiagnostic { kMeshNaive = 0, kMeshWave = 1, kMeshLane = 2 };
static int meshDiagnosticDevice(hpsdf_ctx* ctx, const hpsdf_field* f, MeshDiagnostic which, const double* dXyz, size_t n, double* dOut) {
    static const char* const kRefusal[3] = {"the linear scan is defined for mesh fields", "the shared traversal is defined for mesh fields",
                                            "the per-point traversal is defined for mesh fields"};
    if (f->kind != kHostMesh) return fail(HPSDF_ERR_INVALID_ARGUMENT, kRefusal[which]);
    HPSDF_HIP(hipSetDevice(ctx->device));
    FieldDev fd;
    int rc = makeFieldDev(ctx, f, nullptr, &fd);
    if (rc) return rc;
    if (which == kMeshWave) {
        if (meshFaceRuleReference(ctx))
            return fail(HPSDF_ERR_UNSUPPORTED, "the shared traversal's bounds assume the default face rule (hpsdf_set_mesh_face_rule(0)): use hpsdf_field_eval_* or the scan");
        HPSDF_HIP(launchMeshEvalWave(ctx->stream, fd, dXyz, n, dOut));
        return HPSDF_OK;
    }
    if (which == kMeshLane) {
        HPSDF_HIP(launchFieldEval(ctx->stream, fd, ctx->dTables, dXyz, n, dOut));
        return HPSDF_OK;
    }
    // tiny calls run on the pinned host buffer as the device sees it (hostCall): the scan's atomics then go to the device-side
    // staging buffer, which such a call leaves unused and which holds the call's arrays (32 bytes a point) at least
    unsigned long long* keys = nullptr;
    if (ctx->hostPinDev && (char*)dOut >= ctx->hostPinDev && (char*)dOut < ctx->hostPinDev + ctx->hostPinCap) {
        if (ctx->hostDevCap < n * sizeof(double)) return fail(HPSDF_ERR_STATE, "the staging buffer is smaller than the call");
        keys = reinterpret_cast<unsigned long long*>(ctx->hostDev);
    }
    HPSDF_HIP(launchMeshNaive(ctx->stream, fd, dXyz, n, dOut, keys));
    return HPSDF_OK;
}
static int meshDiagnosticHost(hpsdf_ctx* ctx, const hpsdf_field* f, MeshDiagnostic which, const double* xyz, size_t n, double* out) {
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!f || (!xyz && n) || (!out && n)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return hostRoundTrip(ctx, xyz, n, out, [&](const double* d, double* r) { return meshDiagnosticDevice(ctx, f, which, d, n, r); });
}

int hpsdf_field_eval_wave_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out) {
    HPSDF_TRY
    return meshDiagnosticHost(ctx, f, kMeshWave, xyz, n, out);
    HPSDF_CATCH
}

int hpsdf_field_eval_lane_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out) {
    HPSDF_TRY
    return meshDiagnosticHost(ctx, f, kMeshLane, xyz, n, out);
    HPSDF_CATCH
}

int hpsdf_field_eval_naive_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out) {
    HPSDF_TRY
    return meshDiagnosticHost(ctx, f, kMeshNaive, xyz, n, out);
    HPSDF_CATCH
}

int hpsdf_selftest_acosf(hpsdf_ctx* ctx, uint32_t first_bits, uint32_t stride, size_t n, float* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!out && n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HPSDF_OK;
    HostArrays arr;
    const auto dOut = arr.out(out, n);
    return hostCall(ctx, arr, [&] {
        HPSDF_HIP(launchAcosfSelftest(ctx->stream, first_bits, stride, n, dOut));
        return (int)HPSDF_OK;
    });
    HPSDF_CATCH
}

int hpsdf_selftest_running_total(hpsdf_ctx* ctx, double total0, size_t n, int source, int population, const double* ops, const double* errs,
                                 const double* batch_err, double* out) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    const bool round0 = source == HPSDF_CHAIN_ROUND0;
    if (source != HPSDF_CHAIN_OPS && !round0) return fail(HPSDF_ERR_INVALID_ARGUMENT, "unknown source");
    if (population != HPSDF_CHAIN_ALL_WAVES && population != HPSDF_CHAIN_THIRTEEN_WAVES) return fail(HPSDF_ERR_INVALID_ARGUMENT, "unknown population");
    if (n >= ((size_t)1 << 24)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "n must be below 2^24");
    if (!out || (n && (round0 ? !errs || !batch_err : !ops))) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    // (the call's own arrays in the context's host-call scratch: the frontier workspace of Create is not touched)
    HostArrays arr;
    const auto dOps = arr.in(round0 ? nullptr : ops, round0 ? 0 : n);  // (an array the source does not read: no copy)
    const auto dErrs = arr.in(round0 ? errs : nullptr, round0 ? 9 * n : 0);
    const auto dBatchErr = arr.in(round0 ? batch_err : nullptr, round0 ? n : 0);
    const auto dOut = arr.out(out, 1);
    const HostArrays::Dev<FrHdr> dHdr{arr.add(nullptr, nullptr, sizeof(FrHdr))};  // (scratch: neither copied in nor out)
    return hostCall(ctx, arr, [&] {
        HPSDF_HIP(frLaunchRunningTotal(ctx->stream, dHdr, dOps, dErrs, dBatchErr, total0, (uint32_t)n, round0, population == HPSDF_CHAIN_ALL_WAVES, dOut));
        return (int)HPSDF_OK;
    });
    HPSDF_CATCH
}

}  // extern "C"
