/*
 * hpsdf.h -- C ABI of the MI355X-native hp-adaptive SDF octree hot path.
 *
 * The reference (jw007123/hp-Adaptive-Signed-Distance-Field-Octree) has no FFI
 * or plugin layer: its hot path sits behind the C++ class SDF::Octree
 * (Include/HP/Octree.h:37-86).  This header is the boundary a maintainer binds
 * to replace the bodies of that class's Create / Query / ToMemoryBlock /
 * FromMemoryBlock with gfx950 kernels (the C++ drop-in that
 * does exactly this is include/hpsdf_octree.hpp).
 *
 * Conventions: plain pointers and sizes, POD structs, caller-allocated outputs,
 * no exceptions cross the boundary, every entry point returns an hpsdf_status
 * (0 = ok) and hpsdf_last_error() gives the thread-local message.  Pointers
 * named d_* are device (HBM) pointers on the context's GPU; everything else is
 * host memory.  "stream" is a hipStream_t passed as void*.
 *
 * All file:line citations are relative to the reference checkout.
 */
#ifndef HPSDF_H
#define HPSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define HPSDF_API __attribute__((visibility("default")))
#else
#define HPSDF_API
#endif

typedef enum hpsdf_status {
    HPSDF_OK = 0,
    HPSDF_ERR_INVALID_ARGUMENT = 1,
    HPSDF_ERR_NO_DEVICE = 2,      /* no usable gfx950 device / HIP runtime error */
    HPSDF_ERR_HIP = 3,
    HPSDF_ERR_BAD_BLOCK = 4,      /* malformed MemoryBlock */
    HPSDF_ERR_UNSUPPORTED = 5,
    HPSDF_ERR_STATE = 6,          /* call sequence violated */
    HPSDF_ERR_OUT_OF_MEMORY = 7,
    HPSDF_ERR_OPEN_MESH = 8,      /* Mesh::CreateHalfEdges would return false (Mesh.cpp:121-128) */
    HPSDF_ERR_BUILD_LIMIT = 9     /* Create stopped: the tree outgrew hpsdf_ctx_set_build_limits (ABI 4) */
} hpsdf_status;

/* ---- ABI version ------------------------------------------------------------
 * Bumped whenever a struct of this header changes size or an entry point changes meaning; additions of entry points alone do not
 * bump it.  hpsdf_abi_version() is what the loaded library was built with: a binding compares it with the HPSDF_ABI_VERSION it was
 * compiled against before it hands the library a struct (include/hpsdf_octree.hpp does, and throws on a mismatch).
 *   3 (round 5): hpsdf_build_stats grew from 88 to 112 bytes (fit_mode, split_fits, device_frontier) -- hpsdf_create,
 *                hpsdf_create_distributed and hpsdf_build_get_stats write all 112; hpsdf_ctx_set_fast_fit(ctx, 0) selects
 *                HPSDF_FIT_EXACT (it left HPSDF_FIT_SPLIT on in ABI 2).
 *   4 (round 6): HPSDF_ERR_BUILD_LIMIT; no struct changed.  hpsdf_build_stats is FROZEN at 112 bytes from here on: anything new a
 *                build has to report comes through a getter of its own (hpsdf_ctx_get_build_limits, ...). */
#define HPSDF_ABI_VERSION 4
HPSDF_API int hpsdf_abi_version(void);

/* ---- constants: Include/HP/Consts.h:7-8, Include/HP/Octree.h:89 ----------- */
#define HPSDF_BASIS_MAX_DEGREE 12
#define HPSDF_TREE_MAX_DEPTH 10
#define HPSDF_INTERIOR_DEGREE 13
#define HPSDF_INITIAL_NODE_ERR 100.0
#define HPSDF_DEFAULT_JOBS_PER_ROUND 1024

/* ---- serialised PODs -------------------------------------------------------
 * Byte-identical to the reference structs on Linux LP64, where the reference's
 * "u32" is an 8-byte unsigned long (Include/Utility/Literals.h:9). */

/* SDF::Node, Include/HP/Node.h:10-33 (56 bytes) */
typedef struct hpsdf_node {
    uint64_t child_idx;    /* @0  first of 8 children; all-ones = leaf */
    float aabb_min[3];     /* @8  Eigen::AlignedBox3f min */
    float aabb_max[3];     /* @20 Eigen::AlignedBox3f max */
    uint64_t coeffs_start; /* @32 offset into the coefficient store (doubles) */
    uint8_t degree;        /* @40 13 = interior */
    uint8_t pad0[7];
    uint8_t depth;         /* @48 */
    uint8_t pad1[7];
} hpsdf_node;

/* SDF::Config, Include/HP/Config.h:12-43 (80 bytes) */
typedef struct hpsdf_config {
    uint8_t weighting_type; /* @0  0 None, 1 Polynomial, 2 Exponential */
    uint8_t pad0[7];
    double weighting_strength;  /* @8  */
    uint8_t continuity_enforce; /* @16 */
    uint8_t pad1[7];
    double continuity_strength; /* @24 */
    uint8_t enable_logging;     /* @32 */
    uint8_t pad2[7];
    double target_error_threshold; /* @40 */
    uint64_t thread_count;         /* @48 */
    float root_min[3];             /* @56 */
    float root_max[3];             /* @68 */
} hpsdf_config;

/* Source/HP/Config.cpp:5-14 (thread_count = hardware concurrency) */
HPSDF_API int hpsdf_config_default(hpsdf_config* out);

HPSDF_API const char* hpsdf_last_error(void);
HPSDF_API const char* hpsdf_version(void);

/* ---- constant tables (Include/HP/Utility.h:40-160, Include/HP/Legendre.h) --
 * Copies the host tables the kernels are fed with.  Any pointer may be NULL.
 * roots/weights: 2080 (rule n at n(n-1)/2); normalised_lengths: 13*11;
 * recurrence: 13*2; coeff_count: 13; basis_index: 455*3; sum_to_n: 50. */
HPSDF_API int hpsdf_tables_get(double* roots, double* weights, double* normalised_lengths, double* recurrence,
                               uint64_t* coeff_count, uint64_t* basis_index, uint64_t* sum_to_n);

/* ---- device context --------------------------------------------------------- */
typedef struct hpsdf_ctx hpsdf_ctx;
/* device: HIP ordinal; stream: hipStream_t to launch on (NULL = a stream owned by the context).
 * A context owns the build's workspace (coefficient arena, per-round staging, the continuity post-process's matrix,
 * vectors and worker threads -- all kept between calls): hpsdf_create, the hpsdf_build_* round calls and
 * hpsdf_continuity_post_process_device use one context from one thread at a time.  The *_host query entry points
 * serialise themselves per context (Octree::Query* is const and callable from many threads in the reference);
 * use one context per thread for concurrent builds.
 *
 * The stream contract.  Every *_device entry launches on the context's stream and nowhere else, in the order of the calls: inputs that
 * earlier work on that stream produces are read after it, outputs are complete for later work on that stream, and the context's own
 * scratch is reused in stream order.  Entries documented as asynchronous return without waiting for the stream, with two exceptions
 * that wait on the host because memory changes hands: the first bounds, Integrate, IntegratePair or Clearance call on a tree (it builds
 * the tree's cached constants on the context's stream and waits for them, so that a call on any other stream finds them complete),
 * and a Query on a tree with leaves of degree > 3 that has more points than any such Query of the context before it (the deferred-point
 * scratch is freed and taken again, and freeing device memory waits for the device).  Entries that return host results (Integrate,
 * IntegratePair, Clearance, ClearanceBatch, Simplify, ExtractSurface*, Create, every *_host entry) wait for the stream before they
 * return.  A library-owned stream is non-blocking: it does not synchronise with the null stream.
 *
 * hpsdf_ctx_set_stream moves the context to another stream (NULL: the device's null stream).  Work the context queues afterwards runs
 * behind everything that was queued on the old stream when set_stream was called, the caller's own work included: an event recorded on
 * the old stream is waited for by the new one, with no host wait, so the scratch the two share is never used by both at once.  The old
 * stream must still exist at that moment.  When the old stream is the library-owned one it is synchronised on the host and destroyed
 * instead; the pointer hpsdf_ctx_stream returned before is dead from then on.  The context never owns a stream it was given, and
 * setting the stream it already has (its own included) changes nothing. */
HPSDF_API int hpsdf_ctx_create(int device, void* stream, hpsdf_ctx** out);
HPSDF_API int hpsdf_ctx_destroy(hpsdf_ctx* ctx);
HPSDF_API int hpsdf_ctx_set_stream(hpsdf_ctx* ctx, void* stream);
HPSDF_API int hpsdf_ctx_synchronize(hpsdf_ctx* ctx);
/* How cell fits (Octree::FitPolynomial, Octree.cpp:1007-1093) may leave the reference's term-by-term summation where that changes no
 * decision (csrc/fit_low.hip, csrc/fit_mfma.hip).  A fit's returned error is the sum of squares of its rows of TOP total degree alone (:1062-1069), and the
 * errors are all that selection, the P/H decision (:600-601) and the stop rule (:216) ever read.
 *   HPSDF_FIT_SPLIT (default): a from-scratch fit of degree p >= 6 (hpsdf_ctx_set_split_min_degree) is cut in two -- the rows of total degree p by the term-by-term
 *     kernel that reproduces the reference's summation order bit for bit, the rows below p from the same samples by sum factorisation
 *     (three one-axis contractions with fused multiply-adds: 5-13 x fewer operations than the direct contraction; csrc/fit_low.hip.
 *     HPSDF_LOW_KERNEL=mfma: the direct contraction as a GEMM on the matrix cores instead, v_mfma_f64_16x16x4_f64, degrees >= 4).  Incremental fits (all their rows are top-degree rows) stay exact.  Errors, topology, node array: identical
 *     to HPSDF_FIT_EXACT by construction, no guard band; coefficients of rows below the top degree of leaves that were created by
 *     a split at degree >= 6 agree with it to ~1e-17 absolute (not bit for bit).  Trees whose leaves never exceed degree 5 --
 *     the BASELINE configs stop at 3 -- are byte-identical in both modes.  Weighted builds (the weight reads every row, :1209-1247) and
 *     mesh fits that sample inside the fit kernel keep the exact kernel.
 *   HPSDF_FIT_EXACT: every row by the bit-exact kernel: the canonical bytes (what the CPU oracle produces).
 *   HPSDF_FIT_FAST: every row of every fit of degree >= 4 on the matrix cores.  Errors then agree to ~1e-15 relative only, and
 *     refinement decisions that are exact ties in the reference's arithmetic may fall the other way.
 * hpsdf_ctx_set_fast_fit(ctx, on) = set_fit_mode(on ? HPSDF_FIT_FAST : HPSDF_FIT_EXACT): switching the fast fit off gives the canonical
 * bytes, as it did before the split mode existed (round 5; round 4 sent it to HPSDF_FIT_SPLIT).  The environment variable
 * HPSDF_FIT_MODE=exact|split|fast sets the mode a new context starts with.  hpsdf_build_stats::fit_mode / split_fits say which bytes a
 * build returned: split_fits == 0 means the block is the canonical one whatever the mode. */
enum { HPSDF_FIT_EXACT = 0, HPSDF_FIT_SPLIT = 1, HPSDF_FIT_FAST = 2 };
HPSDF_API int hpsdf_ctx_set_fit_mode(hpsdf_ctx* ctx, int mode);
HPSDF_API int hpsdf_ctx_get_fit_mode(hpsdf_ctx* ctx, int* mode);
/* HPSDF_FIT_SPLIT splits from-scratch fits from this degree on (2..12, 12 = never; default 6, or HPSDF_SPLIT_MIN_DEGREE when the
 * context is created): the two-kernel form pays from degree 5 (-9 %; -27 % / -36 % / -47 % at 6 / 7 / 8), below that the samples' trip
 * through memory costs more than the rows saved (csrc/fit_mfma.hip, fitSplitDefaultMinDegree).  Round 0's coarse fits are never split. */
HPSDF_API int hpsdf_ctx_set_split_min_degree(hpsdf_ctx* ctx, int degree);
HPSDF_API int hpsdf_ctx_set_fast_fit(hpsdf_ctx* ctx, int on);
/* Which way Eigen's 3-vector reductions associate is a property of the reference's BUILD, not of its source: a . (b . c) when Eigen
 * does not vectorise the reduction (EIGEN_DONT_VECTORIZE, non-SSE targets; the default here and in the oracle), (a . b) . c when it
 * reduces a Vector3d through a Packet2d first (what an SSE2 build of Eigen 3.4 appears to do).  Four statements of the path depend on
 * it: aabbScale.prod() (Source/HP/Octree.cpp:1022), unitWeights.prod() (:1040), grad.normalize() (:970) and Vector3d::norm() in the
 * analytic test fields (Source/Tests/HPUnitTests.cpp:48-51; the HPSDF_PRIM_* primitives here).  left_assoc != 0 switches all of them,
 * in every kernel and in the host-answered scalar calls, process-wide and for launches prepared afterwards (call it before Create /
 * Query, not during).  Under either setting the blocks are byte-identical to the oracle's under ora_set_reduction_order() of the same
 * value (tests/test_gpu_parity.py::test_reduction_order_switch_matches_the_oracle).  HPSDF_REDUCTION_ORDER=left sets it at load. */
HPSDF_API void hpsdf_set_reduction_order(int left_assoc);
HPSDF_API int hpsdf_get_reduction_order(void);
/* The same switch for ONE context (round 6): -1 = follow the process-wide setting above (the default), 0 / 1 = this context's own,
 * for every launch it prepares afterwards -- fits, field evaluation, gradient queries, the host-answered scalar calls made through it.
 * Two Octrees of one process can then differ (say, one per reference build being compared against).  _get returns the value in effect. */
HPSDF_API int hpsdf_ctx_set_reduction_order(hpsdf_ctx* ctx, int left_assoc);
HPSDF_API int hpsdf_ctx_get_reduction_order(const hpsdf_ctx* ctx, int* left_assoc);
/* Runaway builds.  The reference's loop (Octree.cpp:212-216) ends when the total error falls below the threshold or the queue is
 * empty; a threshold below what the error estimate can reach on a field (the default Config()'s 1e-10 on most fields, Config.cpp:7)
 * refines towards depth 10 and degree 12 everywhere, and the reference grows its heap until host memory ends.  Here such a build used to
 * end with HPSDF_ERR_OUT_OF_MEMORY when a device allocation finally failed -- minutes later on a 288 GB device.  Limits, checked when
 * a round opens, by both schedulers and by every rank of a sharded build:
 *   max_nodes: the tree's node count (identical on every rank, so every rank stops in the same round);
 *   max_bytes: the device memory this rank's build state needs for the round about to open (node arrays, coefficient arena, sample
 *              buffer -- capacities grow by doubling, so the allocation can reach twice this).
 * 0 = the default: no bound on nodes; bytes = 1/64 of the device memory that is free when the build first needs more than
 * 256 MiB, at least 1 GiB (measured then, once per Create; nothing is measured for builds that stay below, i.e. for every BASELINE
 * config; 4.5 GiB on an idle MI355X -- a tree of one to ten million nodes, which the runaway builds on file reach within 3-15 seconds:
 * profiles/r06_default_config.txt; the first version, 1/256, refused a mesh build at 1e-8 that was most of the way to its threshold).  The hand-over buffer of split fits (HPSDF_FIT_SPLIT) does not count: it is bounded by 2^31 samples
 * (16 GiB) whatever the tree's size.  The DEFAULT bound applies to what grows with the tree -- node arrays and coefficient arena -- and
 * leaves a mesh field's sample buffer out as well (same bound; an ordinary mesh build at 4096 jobs a round needs 1.5-3 GiB of it at
 * degrees 3-4 with a tree of 25 000 nodes); a max_bytes the caller sets bounds all of it.
 * UINT64_MAX = no limit.  A build that crosses a limit returns HPSDF_ERR_BUILD_LIMIT; hpsdf_last_error() names rounds, nodes,
 * bytes, both limits, and the total error against the threshold.  No block is returned.  On several ranks a rank that stops on its
 * bytes alone takes the others out through the FAILURES protocol of hpsdf_create_distributed. */
HPSDF_API int hpsdf_ctx_set_build_limits(hpsdf_ctx* ctx, uint64_t max_nodes, uint64_t max_bytes);
HPSDF_API int hpsdf_ctx_get_build_limits(const hpsdf_ctx* ctx, uint64_t* max_nodes, uint64_t* max_bytes);
HPSDF_API void* hpsdf_ctx_stream(hpsdf_ctx* ctx);

/* ---- fields: the callback F of Octree::Create (Include/HP/Octree.h:50) ------ */
enum { HPSDF_PRIM_SPHERE = 0, HPSDF_PRIM_BOX = 1, HPSDF_PRIM_TORUS_Y = 2, HPSDF_PRIM_PLANE = 3 };
enum { HPSDF_OP_UNION = 0, HPSDF_OP_INTERSECT = 1, HPSDF_OP_SUBTRACT = 2 };
#define HPSDF_MAX_PRIMS 16
typedef struct hpsdf_prim {
    int32_t kind; /* HPSDF_PRIM_* */
    int32_t op;   /* HPSDF_OP_*: how this primitive combines with the running value (ignored for the first) */
    double p[8];  /* sphere: c,r | box: c,half | torus(y axis): c,R,r | plane: n,offset */
} hpsdf_prim;

/* f64 F(const Vector3d& pt, u32 threadIdx): called concurrently from
 * config.thread_count host threads, thread_idx in [0, thread_count)
 * (Source/HP/BuildThreadPool.cpp:10-14). */
typedef double (*hpsdf_callback)(const double* pt, uint64_t thread_idx, void* user);

typedef struct hpsdf_field hpsdf_field;
typedef struct hpsdf_tree hpsdf_tree;

/* evaluated on the GPU inside the fit kernel */
HPSDF_API int hpsdf_field_create_analytic(const hpsdf_prim* prims, int n_prims, hpsdf_field** out);
/* evaluated by host threads per round, values shipped to HBM (keeps Create(config, std::function) working) */
HPSDF_API int hpsdf_field_create_callback(hpsdf_callback cb, void* user, hpsdf_field** out);
/* closed triangle mesh; f32 signed distance with angle-weighted pseudo-normals
 * (Source/Meshing/Mesh.cpp:54-63,162-242; Source/Meshing/Utility.cpp:5-97), evaluated on the GPU
 * over a device BVH.  tris: 3 vertex indices per triangle, CCW. */
HPSDF_API int hpsdf_field_create_mesh(hpsdf_ctx* ctx, const float* verts, uint64_t n_verts, const uint64_t* tris,
                                      uint64_t n_tris, hpsdf_field** out);
/* Meshing::ObjParser::Load (Source/Meshing/ObjParser.cpp:11-164): `v` records and triangular `f` records in
 * the spellings a, a/t, a//n, a/t/n.  *verts (3 floats per vertex) and *tris (3 zero-based indices per
 * triangle) are malloc'd; the caller frees them.  Host-only: needs no device. */
HPSDF_API int hpsdf_obj_load(const char* path, float** verts, uint64_t* n_verts, uint64_t** tris, uint64_t* n_tris);
/* F'(p) = op(old.Query(p), inner(p)): Octree::UnionSDF/SubtractSDF/IntersectSDF, Octree.cpp:355-400.
 * op: HPSDF_OP_UNION -> min(old,F); HPSDF_OP_SUBTRACT -> max(-old,F); HPSDF_OP_INTERSECT -> max(old,F). */
HPSDF_API int hpsdf_field_create_tree_csg(const hpsdf_tree* old_tree, int op, const hpsdf_field* inner,
                                          hpsdf_field** out);
HPSDF_API int hpsdf_field_destroy(hpsdf_field* f);
/* F at n world-space points (device pointers, xyz interleaved); analytic/mesh/tree fields only. */
HPSDF_API int hpsdf_field_eval_device(hpsdf_ctx* ctx, const hpsdf_field* f, const double* d_xyz, size_t n,
                                      double* d_out);
HPSDF_API int hpsdf_field_eval_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out);
/* Calls of one or two points on a plain mesh field (Mesh::SignedDistanceAtPt(pt, bvh) from a user's SDF lambda) are answered on the
 * calling thread from host copies of the field's device-built arrays.  The first such call makes them: one device-wide
 * synchronisation and a download of the whole mesh (vertices, triangles, records, BVH: ~160 bytes a triangle), kept until the field is
 * destroyed or this call drops them.  Meshes whose copies would exceed HPSDF_HOST_MESH_MIRROR_MB (default 512) are never mirrored:
 * their small calls are launches. */
HPSDF_API int hpsdf_field_release_host_copies(hpsdf_field* f);
/* Mesh fields, the one stated deviation from the reference's closest-point arithmetic (Source/Meshing/Utility.cpp:5-97): its face
 * case returns q = u a + v b + w c whatever the barycentric weights are, and beside the short edges of needle-shaped triangles
 * (its 1e-6 guards are absolute) a weight can be negative enough to put q well outside the triangle -- a distance below the
 * triangle's own, which a search reports or not depending on what it has pruned (the reference's BVH and its linear scan
 * disagree there too).  Here a face-case point farther outside its triangle than 5e-7 of the mesh's scale (a quarter of the
 * traversal's slack) is not taken by a search it could win: the closest point of the triangle's boundary (the nearest of its three
 * edges' closest points, f32) takes its place.  Consequences: the four evaluation paths
 * below (naive scan, per-lane traversal, shared traversal, hpsdf_field_eval_*) agree BIT FOR BIT on every mesh; against the
 * reference's arithmetic they differ exactly at the points where its own value is such an artefact (6 points in 8 000 random
 * meshes x 5 301 points, all on meshes squashed 100 : 1 or more; tests/test_gpu_configs.py::test_needle_meshes_one_answer_on_every_path).
 * At such a point the value is the distance to the triangle's boundary: at least the true distance, and above it by a fraction of the
 * needle's width when the true closest point lies inside the needle (largest seen in the sweeps: 2.9e-4 of the mesh's extent, where the
 * reference's value was 4e-3 of the extent BELOW the distance; tools/fuzz_mesh_bvh.py, seed 910968). */
/* ... and the way back to the reference's values: hpsdf_set_mesh_face_rule(1) (process-wide, for launches prepared afterwards; the
 * environment variable HPSDF_MESH_FACE_RULE=reference sets it from the start) makes the closest-point routine return Utility.cpp:5-97's
 * face-case point unconditionally.  The O(n) scan (hpsdf_field_eval_naive_host) then equals the reference's Mesh::SignedDistanceAtPt(pt),
 * Mesh.cpp:134-159, operation by operation on every mesh, needles included; hpsdf_field_eval_* and mesh builds use the per-point
 * traversal, which prunes by boxes only, as the reference's BVH does -- and, like it, may report such an artefact or not depending
 * on what it pruned.  The shared traversal (hpsdf_field_eval_wave_host, and the sampler of the device-side frontier) bounds distances
 * to TRIANGLES, which an artefact can undercut: it returns HPSDF_ERR_UNSUPPORTED under this rule, and Create with a mesh field takes
 * the host scheduler with the per-point traversal inside the fit (what HPSDF_MESH_FUSED=1 selects). */
HPSDF_API void hpsdf_set_mesh_face_rule(int reference);
HPSDF_API int hpsdf_get_mesh_face_rule(void);
/* ... per context (round 6): -1 = follow the process-wide rule (default), 0 / 1 = this context's own, for the launches it prepares. */
HPSDF_API int hpsdf_ctx_set_mesh_face_rule(hpsdf_ctx* ctx, int reference);
HPSDF_API int hpsdf_ctx_get_mesh_face_rule(const hpsdf_ctx* ctx, int* reference);
/* (Mesh fields: a point with a coordinate that is not a finite number has no closest triangle -- the reference's search ends
 * with bestTri = -1 there and reads out of bounds, Mesh.cpp:139,157 -- and evaluates to a NaN on every entry point below.) */
/* Mesh::SignedDistanceAtPt(pt) without a BVH (Source/Meshing/Mesh.cpp:42-51 over the O(n) scan :134-159), mesh fields
 * only: every triangle is tested for every point (one wave per point).  What the reference's TestBVHQuerying
 * (Source/Tests/MeshingUnitTests.cpp:110-138) compares the BVH answer with; same tie rule, so the two agree bit for bit. */
HPSDF_API int hpsdf_field_eval_naive_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out);
/* Mesh::SignedDistanceAtPt(pt, bvh, threadIdx) (Source/Meshing/Mesh.cpp:54-84) through the traversal Create's sampler
 * uses: 64 points share one walk of the BVH.  Same values as hpsdf_field_eval_host bit for bit, whatever the order of the
 * points: sets of 4096 points or more are visited along a Morton curve (an index sort on the device), so that a wave's
 * points are neighbours in space even when the array's are not.  Mesh fields only. */
HPSDF_API int hpsdf_field_eval_wave_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out);
/* The same through the per-point stack traversal (what a mesh field under a tree-CSG wrapper and the fused mesh fit run;
 * hpsdf_field_eval_* itself takes the faster shared traversal for plain mesh fields): same bits.  Diagnostics. */
HPSDF_API int hpsdf_field_eval_lane_host(hpsdf_ctx* ctx, const hpsdf_field* f, const double* xyz, size_t n, double* out);
/* Diagnostics: the device's acosf -- the angle weights of a vertex pseudo-normal, std::acos in Source/Meshing/Mesh.cpp:226-231
 * -- for the n floats whose bit patterns are first_bits, first_bits + stride, ...  It is glibc's float acos as shipped up to glibc
 * 2.40 (the fdlibm e_acosf algorithm, restated in csrc/acosf_host_libm.hpp): out[] equals acosf() of such a host bit for bit.
 * glibc >= 2.41 (correctly rounded CORE-MATH acosf), musl and other libms may differ from it in the last place; the tests
 * detect that (tests/test_product_cpu.py compares with the machine's libm and says which one it found). */
HPSDF_API int hpsdf_selftest_acosf(hpsdf_ctx* ctx, uint32_t first_bits, uint32_t stride, size_t n, float* out);
/* Diagnostics: the running total of Create's stop rule (Octree.cpp:253-290) on operands of the caller's choice -- the device code
 * Create itself runs (one workgroup; four additions an instruction on the matrix pipe), not a copy of it.  *out = total0 + x[0] + x[1]
 * + ... + x[n - 1], one IEEE double addition after the other in that order: bit for bit what a sequential loop on the host gives
 * (tests/test_gpu_running_total.py holds it to that).  source HPSDF_CHAIN_OPS: x = ops[0 .. n) (rounds >= 1); HPSDF_CHAIN_ROUND0:
 * x[k] = errs[9 k] - batch_err[k], formed on the device as round 0 does (errs holds 9 n doubles, batch_err n); the arrays of the
 * other source are not read and may be NULL.  population: all sixteen waves of the workgroup take part, as where round 0's total is added
 * up, or thirteen (waves 4, 8 and 12 have left), as in later rounds.  n = 0 gives total0; n >= 2^24, an unknown source or population, a
 * NULL out or a NULL array the source reads with n > 0: HPSDF_ERR_INVALID_ARGUMENT, *out untouched.  Leaves Create's state alone. */
enum { HPSDF_CHAIN_OPS = 0, HPSDF_CHAIN_ROUND0 = 1 };
enum { HPSDF_CHAIN_ALL_WAVES = 0, HPSDF_CHAIN_THIRTEEN_WAVES = 1 };
HPSDF_API int hpsdf_selftest_running_total(hpsdf_ctx* ctx, double total0, size_t n, int source, int population, const double* ops,
                                           const double* errs, const double* batch_err, double* out);
/* Diagnostics (no reference counterpart; HPSDF_ERR_UNSUPPORTED unless the library was built with
 * -DHPSDF_MESH_STATS_BUILD): BVH traversal counters of a mesh field created while the environment
 * variable HPSDF_MESH_STATS was set -- out[0] wave-wide closest-triangle queries (64 points each), [1] BVH nodes they visited,
 * [2] (point, triangle) pairs that went through the lower-bound test, [3] pairs that went on to the closest-point test,
 * [4] (point, leaf) pairs queued, [5] wave-wide batches of lower-bound tests, [6] of closest-point tests, [7] points whose
 * seed (the leaf their own descent ended in) already held the answer.  Synchronises the device; reset != 0 zeroes the counters. */
HPSDF_API int hpsdf_field_mesh_stats(const hpsdf_field* f, uint64_t out[8], int reset);
/* Diagnostics (no reference counterpart; read-only): what a mesh field keeps on the device, copied to the host after a device-wide
 * synchronisation -- the data every traversal prunes by (csrc/device_types.hpp has the layouts).  info[0..4] = vertices, triangles, BVH
 * nodes, log2 of the largest leaf, 1 if the field has slabs.  buffers (null: only info is filled) and capacities (bytes) have seven
 * entries: verts (3 f32 per vertex), tris (3 u32 per triangle), triPos and triPre (12 f32 per triangle / per leaf slot), halfEdges
 * (3 u32 per triangle), bvh and slabs (64 bytes per BVH node); a null entry is skipped, the slabs' entry also when the field has none.
 * HPSDF_ERR_INVALID_ARGUMENT for a field that is not a mesh and for a buffer smaller than its array: nothing is written then. */
HPSDF_API int hpsdf_field_mesh_arrays(const hpsdf_field* f, uint64_t info[5], void* const* buffers, const uint64_t* capacities);

/* ---- Query: Octree::FromMemoryBlock + Octree::Query (Octree.cpp:403-421, 662-702, 859-901) */
/* block layout: [u64 nCoeffs][f64 x nCoeffs][u64 nNodes][hpsdf_node x nNodes][hpsdf_config] */
HPSDF_API int hpsdf_tree_upload(hpsdf_ctx* ctx, const void* block, size_t size, hpsdf_tree** out);
HPSDF_API int hpsdf_tree_destroy(hpsdf_tree* t);
HPSDF_API int hpsdf_tree_info(const hpsdf_tree* t, uint64_t* n_nodes, uint64_t* n_coeffs, uint64_t* n_leaves,
                              int* max_degree, int* max_depth);
/* out[i] = Query(xyz[3i..3i+2]); DBL_MAX outside the root (Octree.cpp:668-671).
 * Asynchronous on the context stream; no host synchronisation. */
HPSDF_API int hpsdf_query_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_xyz, size_t n, double* d_out);
/* host buffers: H2D + kernel + D2H, synchronous (PCIe-inclusive) */
HPSDF_API int hpsdf_query_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double* out);

/* Octree::QueryWithGradient (Octree.cpp:749-789, 904-985): out[i] as Query; grad[3i..] = the reference's
 * normalised central-difference "gradient".  Rows of points outside the root are left untouched. */
HPSDF_API int hpsdf_query_gradient_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_xyz, size_t n,
                                          double* d_out, double* d_grad);
HPSDF_API int hpsdf_query_gradient_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double* out,
                                        double* grad);

/* ---- QueryGradient: the value and the gradient of the polynomial the value comes from (no reference counterpart).
 * QueryWithGradient above reproduces the reference's shortcut: per axis k it differences sum_r c_r Lhat_{idx[r][k]}(u_k +- 1e-4), which
 * leaves the other two axes' factors of every basis function out -- it is not the derivative of Query.  This call is.
 *
 * The arithmetic, for host and device alike (no fused multiply-add anywhere; every sum starts from 0.0 and runs in basis order):
 *   Query's own remap (Octree.cpp:665), f32 containment test (:668) and descent (:674-701; a point on a mid-plane takes the upper
 *   child, so on a cell face the gradient is that of the leaf Query answers from).  In the leaf -- degree p, depth d, unit coordinates
 *   u = (pt - centre) * (2 << d) as Octree.cpp:862 -- per axis a:
 *     L_j(u_a), j <= p      the recurrence of Query with its constants: L_0 = 1, L_j = rec[j][0] u L_{j-1} - rec[j][1] L_{j-2}
 *     D_0 = 0, D_1 = 1, D_j = D_{j-2} + (double)(2j-1) L_{j-1}  for j >= 2      (= L_j')
 *     LN_j = L_j nl[j][d],  DN_j = D_j nl[j][d]
 *   value   f      Query's statements exactly: f += c_r ((LN_a(x) LN_b(y)) LN_c(z)) over rows r = (a,b,c) -- hpsdf_query_*'s bits
 *   unit-space partials, over the same rows:
 *     gu_0 += c_r ((DN_a(x) LN_b(y)) LN_c(z)),  gu_1 += c_r ((LN_a DN_b) LN_c),  gu_2 += c_r ((LN_a LN_b) DN_c)
 *   world gradient  g_a = (gu_a (double)(2 << d)) rootInvSizes[a]   (the chain rule through :862 and :665; the first factor is a power
 *     of two, the second the f32-derived reciprocal the tree holds, so anisotropic roots are handled)
 *   HPSDF_GRADIENT_UNIT: z = g_0^2 + (g_1^2 + g_2^2), or (g_0^2 + g_1^2) + g_2^2 under hpsdf_[ctx_]set_reduction_order(1); if z > 0,
 *     g_a = g_a / sqrt(z); otherwise the row stays as computed (zeros).
 *   Outside the root, or a NaN coordinate: value DBL_MAX, gradient row three quiet NaNs (this call is new: it does not inherit
 *   QueryWithGradient's "left untouched").
 * out may be NULL (gradients only).  Unknown flag bits, a NULL grad with n > 0 or a NULL tree: HPSDF_ERR_INVALID_ARGUMENT.  n == 0 is
 * HPSDF_OK.  _device is asynchronous on the context stream; _host answers calls of up to 32 points on the calling thread
 * (csrc/host_query.cpp) and sends larger ones through the device; _block needs no device at all: it evaluates from a serialised
 * block on the calling thread, under the process-wide reduction order.  It accepts exactly the blocks hpsdf_tree_upload accepts, with
 * upload's status for the others: HPSDF_ERR_BAD_BLOCK for a malformed block (a root without its 8 children included),
 * HPSDF_ERR_UNSUPPORTED for a root box other than [-0.5,0.5]^3 or child boxes that are not midpoint octants.  All three give the
 * same bits. */
#define HPSDF_GRADIENT_UNIT 1u
HPSDF_API int hpsdf_query_true_gradient_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_xyz, size_t n, uint32_t flags,
                                               double* d_out, double* d_grad);
HPSDF_API int hpsdf_query_true_gradient_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, uint32_t flags,
                                             double* out, double* grad);
HPSDF_API int hpsdf_query_true_gradient_block(const void* block, size_t size, const double* xyz, size_t n, uint32_t flags, double* out,
                                              double* grad);

/* ---- QueryHessian: the value, the gradient and the second derivative of the polynomial the value comes from, and the mean and
 * Gaussian curvature of its level set through the point (no reference counterpart).
 *
 * The arithmetic, for host and device alike (no fused multiply-add anywhere; every sum starts from 0.0 and runs in basis order):
 *   Query's own remap, f32 containment test and descent (a point on a mid-plane takes the upper child).  In the leaf -- degree p, depth
 *   d, unit coordinates u and the table nl as in QueryGradient -- per axis a:
 *     L_j, D_j, LN_j, DN_j    exactly QueryGradient's
 *     E_0 = E_1 = 0,  E_j = E_{j-2} + (double)(2j-1) D_{j-1}  for j >= 2      (= L_j'')
 *     EN_j = E_j nl[j][d]
 *   over rows r = (a,b,c):
 *     f       Query's bits, and gu_0..2 QueryGradient's bits: the same statements in the same order
 *     hu_xx += c_r ((EN_a LN_b) LN_c),  hu_yy += c_r ((LN_a EN_b) LN_c),  hu_zz += c_r ((LN_a LN_b) EN_c)
 *     hu_xy += c_r ((DN_a DN_b) LN_c),  hu_xz += c_r ((DN_a LN_b) DN_c),  hu_yz += c_r ((LN_a DN_b) DN_c)
 *   world Hessian, with s = (double)(2 << d):  H_ab = (((hu_ab s) s) rootInvSizes[a]) rootInvSizes[b]
 *     hess holds 6 doubles per point in the order xx, yy, zz, xy, xz, yz.
 *   world gradient g: QueryGradient's, not normalised.  HPSDF_GRADIENT_UNIT in flags normalises only the gradient row that is written
 *     out; the curvature always uses the un-normalised g.
 *   curvature, curv[2] = (mean, gauss), with sum3(a,b,c) = a + (b + c), or (a + b) + c under hpsdf_[ctx_]set_reduction_order(1):
 *     z = sum3(g0 g0, g1 g1, g2 g2);  if !(z > 0): both entries are quiet NaN
 *     Hg_a = sum3(H_a0 g0, H_a1 g1, H_a2 g2);  q = sum3(g0 Hg_0, g1 Hg_1, g2 Hg_2);  tr = sum3(H_xx, H_yy, H_zz)
 *     mean = (z tr - q) / ((2.0 z) sqrt(z))
 *     A00 = Hyy Hzz - Hyz Hyz,  A11 = Hxx Hzz - Hxz Hxz,  A22 = Hxx Hyy - Hxy Hxy
 *     A01 = Hxz Hyz - Hxy Hzz,  A02 = Hxy Hyz - Hxz Hyy,  A12 = Hxy Hxz - Hxx Hyz        (A symmetric)
 *     Ag_a = sum3(A_a0 g0, A_a1 g1, A_a2 g2);  k = sum3(g0 Ag_0, g1 Ag_1, g2 Ag_2);  gauss = k / (z z)
 *     Sign convention: with the field positive outside, a sphere of radius r has mean = 1/r and gauss = 1/r^2.
 *   Outside the root, or a NaN coordinate: the value is DBL_MAX and every other output row is quiet NaNs.
 * Caveat: the field is piecewise polynomial and discontinuous across cell faces, and so are its derivatives.  Leaves of degree <= 1 have
 * a zero Hessian and leaves of degree 2 a constant one; trees built at the default thresholds hold leaves of degree <= 2 only, so the
 * curvature they give is crude.  Curvature is meaningful on refined trees (smaller targets, higher degrees).
 * Each of out, grad, hess and curv may be NULL, but hess and curv must not both be NULL.  Unknown flag bits, a NULL tree, or NULL points
 * with n > 0: HPSDF_ERR_INVALID_ARGUMENT, and nothing is written.  n == 0 is HPSDF_OK.  _device is asynchronous on the context stream;
 * _host answers calls of up to 32 points on the calling thread (csrc/host_query.cpp) and sends larger ones through the device; _block
 * needs no device: it evaluates from a serialised block on the calling thread under the process-wide reduction order, and accepts and
 * refuses blocks exactly as hpsdf_query_true_gradient_block does.  All three give the same bits. */
HPSDF_API int hpsdf_query_hessian_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_xyz, size_t n, uint32_t flags, double* d_out,
                                         double* d_grad, double* d_hess, double* d_curv);
HPSDF_API int hpsdf_query_hessian_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, uint32_t flags, double* out,
                                       double* grad, double* hess, double* curv);
HPSDF_API int hpsdf_query_hessian_block(const void* block, size_t size, const double* xyz, size_t n, uint32_t flags, double* out, double* grad,
                                        double* hess, double* curv);

/* ---- ProjectToSurface: Newton's iteration along the gradient onto the level set {Query = iso} (no reference counterpart).
 * Per point, with iso finite, tol >= 0 (not NaN) and max_iter in 0..255; host, device and block entries run the same statements (no
 * fused multiply-add anywhere) and give the same bits:
 *     x = input point;  k = 0
 *     loop:
 *       (f, g) = QueryGradient(x), the world gradient, not normalised -- the statements stated above
 *       if f == DBL_MAX (x outside the root, or a NaN coordinate):   status = HPSDF_PROJECT_LEFT_ROOT;   stop
 *       r = f - iso
 *       if fabs(r) <= tol:                                           status = HPSDF_PROJECT_CONVERGED;   stop
 *       a = g_0 g_0, b = g_1 g_1, c = g_2 g_2;  z = a + (b + c), or (a + b) + c under hpsdf_[ctx_]set_reduction_order(1)
 *       if !(z > 0):                                                 status = HPSDF_PROJECT_FLAT;        stop
 *       if k == max_iter:                                            status = HPSDF_PROJECT_ITER_LIMIT;  stop
 *       s = r / z;   x_a = x_a - s g_a  (a = 0, 1, 2);   k = k + 1
 * Outputs per point, every one except out_xyz optional (NULL):
 *   out_xyz[3]   the x at which the loop stopped (LEFT_ROOT: the position outside the root; a NaN input: the input as it is)
 *   out_val      f there;   out_grad[3]  g there, normalised as HPSDF_GRADIENT_UNIT normalises it under HPSDF_PROJECT_UNIT; three quiet
 *                NaNs for LEFT_ROOT.  Hence (out_val, out_grad) is QueryGradient(out_xyz) bit for bit on every row.
 *   out_iters    k (uint8_t);   out_status  the status (uint8_t)
 * out_xyz may be the input array itself (a point is read before its row is written).
 * There is no damping, no step clamp and no line search, and the result is where the gradient lines lead, not a guaranteed closest
 * point.  The field is piecewise polynomial and discontinuous across cell faces: near creases and the medial axis the iteration can
 * hop between two cells for ever, each cell's polynomial sending the point back into the other.  HPSDF_PROJECT_ITER_LIMIT reports
 * that (or a max_iter too small); the row then holds the last position reached.  (A step that overflows can produce a NaN coordinate;
 * the next turn stops with LEFT_ROOT, and the bits of such a NaN are the platform's.)
 * Unknown flag bits, a NULL out_xyz (or input) with n > 0, a NULL tree, tol negative or NaN, a non-finite iso, max_iter > 255:
 * HPSDF_ERR_INVALID_ARGUMENT, and no output is written.  n == 0 is HPSDF_OK.  _device is asynchronous on the context stream; _host
 * answers calls of up to 32 points on the calling thread and sends larger ones through the device; _block needs no device: it works
 * from a serialised block on the calling thread under the process-wide reduction order, and accepts and refuses blocks as
 * hpsdf_tree_upload does (malformed: HPSDF_ERR_BAD_BLOCK; boxes the descent would not recompute: HPSDF_ERR_UNSUPPORTED). */
#define HPSDF_PROJECT_UNIT 1u
enum { HPSDF_PROJECT_CONVERGED = 0, HPSDF_PROJECT_ITER_LIMIT = 1, HPSDF_PROJECT_LEFT_ROOT = 2, HPSDF_PROJECT_FLAT = 3 };
HPSDF_API int hpsdf_project_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_xyz, size_t n, double iso, double tol,
                                   uint32_t max_iter, uint32_t flags, double* d_out_xyz, double* d_out_val, double* d_out_grad,
                                   uint8_t* d_out_iters, uint8_t* d_out_status);
HPSDF_API int hpsdf_project_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* xyz, size_t n, double iso, double tol, uint32_t max_iter,
                                 uint32_t flags, double* out_xyz, double* out_val, double* out_grad, uint8_t* out_iters,
                                 uint8_t* out_status);
HPSDF_API int hpsdf_project_block(const void* block, size_t size, const double* xyz, size_t n, double iso, double tol, uint32_t max_iter,
                                  uint32_t flags, double* out_xyz, double* out_val, double* out_grad, uint8_t* out_iters,
                                  uint8_t* out_status);
/* Marching-cubes vertices are linear interpolants along lattice edges and do not lie on the polynomial's level set.  This call moves
 * the nv vertices of verts (host, 3 doubles each, in place) onto it: every vertex goes through hpsdf_project_host (flags 0), and vertex
 * i is replaced by its projection only if its status is HPSDF_PROJECT_CONVERGED and fabs(projected_a - vertex_a) <= 0.5 * h[a] on every
 * axis a, h being the cube size of the lattice the mesh was extracted on ((hi[a] - lo[a]) / n[a] of hpsdf_extract_surface).  Any other
 * vertex stays exactly as it was, so the triangle list stays valid and no vertex moves far enough to fold its triangles.  *n_moved
 * (may be NULL): how many vertices were replaced.  A NULL verts with nv > 0, a NULL h or an h[a] that is negative or NaN, and
 * whatever hpsdf_project_host rejects: HPSDF_ERR_INVALID_ARGUMENT, verts untouched. */
HPSDF_API int hpsdf_surface_project_vertices(hpsdf_ctx* ctx, const hpsdf_tree* t, double* verts, uint64_t nv, const double h[3], double iso,
                                             double tol, uint32_t max_iter, uint64_t* n_moved);

/* ---- CastRays: the first crossing of a ray with the level set {Query = iso} (no reference counterpart; hpsdf_query_ray_* below stays
 * the reference's sphere tracing, statement by statement).  The field is a polynomial of total degree <= p inside a leaf, hence a
 * polynomial of degree <= p in the ray parameter there: the ray is walked leaf by leaf, sampled max(1, p) times per leaf segment, and
 * the first sign change of Query - iso is refined by a safeguarded Newton iteration on the polynomial's own directional derivative.
 * There is no distance-field (Lipschitz) assumption and no fixed epsilon.
 * Per ray: a world origin o[3], a world direction d[3] used as it is (t is in units of |d|), t_max; per call iso (finite), tol (>= 0,
 * not NaN), max_iter (0..255), max_cells (1..65535).  Host, device and block entries run the same statements (csrc/ray_cast.hpp; no
 * fused multiply-add anywhere) and give the same bits.  With
 *     x(t)_a = o_a + t d_a                       (one multiply, one add)
 *     (f, g)(t) = QueryGradient(x(t)), the world gradient, not normalised;   r(t) = f - iso
 *     s(t) = sum3(g_0 d_0, g_1 d_1, g_2 d_2),  sum3(a,b,c) = a + (b + c), or (a + b) + c under hpsdf_[ctx_]set_reduction_order(1)
 *     below(v) = the largest double less than v
 *   1 validity   a non-finite o_a or d_a, d = 0 on all axes, t_max NaN or negative:                    status = HPSDF_CAST_INVALID
 *   2 clip       ou_a = (o_a - rootCentre_a) rootInvSizes_a;  du_a = d_a rootInvSizes_a;  t0 = 0;  t1 = t_max;  per axis a = 0, 1, 2:
 *                  du_a == 0:  if !(-0.5 <= ou_a <= 0.5):                                              status = HPSDF_CAST_MISS
 *                  else  tl = (-0.5 - ou_a) / du_a,  th = (0.5 - ou_a) / du_a;  (tin, tout) = du_a > 0 ? (tl, th) : (th, tl)
 *                        if tin > t0: t0 = tin;   if tout < t1: t1 = tout
 *                if !(t0 <= t1):                                                                       status = HPSDF_CAST_MISS
 *   3 first      te = t0; evaluate (every evaluation counts one in out_evals):
 *                  f == DBL_MAX (the point rounded outside the root):                                  status = HPSDF_CAST_MISS
 *                  prev = r(t0), t_prev = t0;  fabs(prev) <= tol:                                      status = HPSDF_CAST_HIT at t0
 *   4 walk       pu_a = ou_a + t0 du_a (the product first) clamped into [-0.5, 0.5];  Query's descent of pu gives the leaf: its box
 *                [lo_a, hi_a] (exact dyadics) and degree p;  cells = 1;  t = t0.  Then repeat:
 *       exit     over the axes with du_a != 0 in the order 0, 1, 2:  face_a = du_a > 0 ? hi_a : lo_a,  ta = (face_a - ou_a) / du_a;
 *                tb = the smallest ta, e = the first axis attaining it (no such axis: tb = t1, and the move below is a MISS);
 *                if !(tb >= t): tb = t;   if !(tb <= t1): tb = t1
 *       samples  if tb > t:  S = max(1, p);  for j = 1..S:  t_j = t + (tb - t) ((double)j / (double)S), and t_S = tb itself;
 *                  f == DBL_MAX:                                                                       status = HPSDF_CAST_MISS
 *                  cur = r(t_j);  fabs(cur) <= tol:                                                    status = HPSDF_CAST_HIT at t_j
 *                  (prev < 0) != (cur < 0):  refine the bracket [t_prev, t_j] (step 5)
 *                  else prev = cur, t_prev = t_j
 *       end      if tb >= t1:                                                                          status = HPSDF_CAST_MISS
 *       move     across face e:  du_e > 0 and hi_e >= 0.5, or du_e < 0 and lo_e <= -0.5 (the root's own face):  status = HPSDF_CAST_MISS
 *                if cells == max_cells:                                                                status = HPSDF_CAST_CELL_LIMIT
 *                pu_e = du_e > 0 ? hi_e : below(lo_e)      (the descent's >= takes the upper cell at the face itself)
 *                pu_a = ou_a + tb du_a clamped into [lo_a, below(hi_a)] on the other two axes
 *                descend pu to the next leaf;  cells = cells + 1;  t = tb
 *                Every move crosses one cell face in the direction of travel, so the walk always advances.
 *   5 refine     [a, b] = [t_prev, t_j]: r(a) and r(b) of opposite sign, neither within tol.  c = b;  k = 0;  halved = true.  Repeat:
 *                  tn = c - r(c) / s(c);   m = tn if halved and a < tn < b, else a + 0.5 (b - a)
 *                  if !(a < m < b) or k == max_iter:                                                   status = HPSDF_CAST_UNCONVERGED at b
 *                  evaluate at m;  f == DBL_MAX:                                                       status = HPSDF_CAST_UNCONVERGED at b
 *                  fabs(r(m)) <= tol:                                                                  status = HPSDF_CAST_HIT at m
 *                  w = b - a;  the end of the bracket whose r has the sign of r(m) (sign: r < 0) becomes m;  c = m
 *                  halved = (b - a) <= 0.5 w;   k = k + 1
 * HPSDF_CAST_UNCONVERGED is an outcome, not an error: the field jumps across cell faces, and a sign change can sit on a jump wider
 * than tol; the row then holds the upper end of the last bracket (the first sample behind the crossing).
 * Outputs per ray; out_status is required, every other output optional (NULL):
 *   out_status   uint8_t, HPSDF_CAST_*
 *   out_t        the parameter of the row; a quiet NaN for MISS, INVALID and CELL_LIMIT
 *   out_xyz[3]   x(out_t); quiet NaNs where out_t is one
 *   out_val, out_grad[3]   QueryGradient(out_xyz) bit for bit (DBL_MAX and quiet NaNs where out_xyz is NaN); under HPSDF_CAST_UNIT the
 *                gradient is normalised as HPSDF_GRADIENT_UNIT normalises it
 *   out_evals    uint16_t, field evaluations spent (saturating at 65535);   out_cells   uint16_t, leaves visited
 * Limits: two crossings closer together than one sample interval (a grazing ray) are not seen; a crossing that exists only as a jump
 * across a cell face is reported as HPSDF_CAST_UNCONVERGED; the samples are placed by the walk's own arithmetic, while each one is
 * evaluated by the ordinary descent of x(t), so a sample within rounding of a cell face may be answered by the neighbouring leaf.
 * Unknown flag bits, a NULL tree, NULL origins, dirs, t_max or out_status with n > 0, tol negative or NaN, a non-finite iso,
 * max_iter > 255, max_cells outside 1..65535: HPSDF_ERR_INVALID_ARGUMENT, and no output is written.  n == 0 is HPSDF_OK.  _device is
 * asynchronous on the context stream; _host answers calls of up to 32 rays on the calling thread and sends larger ones through the
 * device; _block needs no device: it works from a serialised block on the calling thread under the process-wide reduction order, and
 * accepts and refuses blocks as hpsdf_project_block does. */
#define HPSDF_CAST_UNIT 1u
enum { HPSDF_CAST_HIT = 0, HPSDF_CAST_MISS = 1, HPSDF_CAST_UNCONVERGED = 2, HPSDF_CAST_CELL_LIMIT = 3, HPSDF_CAST_INVALID = 4 };
HPSDF_API int hpsdf_cast_rays_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_origins, const double* d_dirs, const double* d_t_max,
                                     size_t n, double iso, double tol, uint32_t max_iter, uint32_t max_cells, uint32_t flags,
                                     uint8_t* d_out_status, double* d_out_t, double* d_out_xyz, double* d_out_val, double* d_out_grad,
                                     uint16_t* d_out_evals, uint16_t* d_out_cells);
HPSDF_API int hpsdf_cast_rays_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* origins, const double* dirs, const double* t_max, size_t n,
                                   double iso, double tol, uint32_t max_iter, uint32_t max_cells, uint32_t flags, uint8_t* out_status,
                                   double* out_t, double* out_xyz, double* out_val, double* out_grad, uint16_t* out_evals,
                                   uint16_t* out_cells);
HPSDF_API int hpsdf_cast_rays_block(const void* block, size_t size, const double* origins, const double* dirs, const double* t_max, size_t n,
                                    double iso, double tol, uint32_t max_iter, uint32_t max_cells, uint32_t flags, uint8_t* out_status,
                                    double* out_t, double* out_xyz, double* out_val, double* out_grad, uint16_t* out_evals,
                                    uint16_t* out_cells);

/* Octree::QueryRay (Octree.cpp:705-746; Ray: Include/HP/Ray.h, Source/HP/Ray.cpp:5-68) for n rays: sphere
 * tracing, <= 200 Query steps each.  hit[i] = 1/0; t[i] is written only on a hit (the reference leaves t_
 * untouched otherwise) and receives what the reference stores there -- the field value at the stopping point
 * (Octree.cpp:730).  origins/dirs: xyz interleaved, world coordinates; dirs are used as given.  A _host call of up to 32 rays -- the
 * scalar QueryRay(ray, tMax, t) -- is stepped on the calling thread like the scalar Query (csrc/host_query.cpp): same bits, no launch. */
HPSDF_API int hpsdf_query_ray_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_origins,
                                     const double* d_dirs, const double* d_tmax, size_t n, uint8_t* d_hit,
                                     double* d_t);
HPSDF_API int hpsdf_query_ray_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* origins, const double* dirs,
                                   const double* tmax, size_t n, uint8_t* hit, double* t_out);

/* Octree::OutputFunctionSlice (Octree.cpp:1131-1206) up to the byte image: n_samples^2 Query() calls on the
 * plane z = c over [view_min.xy, view_min.xy + (view_max.x - view_min.x)) (the reference steps both axes by
 * the x extent), then its green/blue normalisation.  rgb: n_samples^2 * 3 bytes, row i = y index (host);
 * values: the n_samples^2 Query results (host, may be NULL).  The reference uses n_samples = 2048 and hands
 * the bytes to stb_image_write (not a dependency here; include/hpsdf_octree.hpp writes the BMP itself). */
HPSDF_API int hpsdf_function_slice(hpsdf_ctx* ctx, const hpsdf_tree* t, double c, const float* view_min,
                                   const float* view_max, uint64_t n_samples, uint8_t* rgb, double* values);

/* ---- ExtractSurface: marching cubes over a lattice of Query values (no reference counterpart) ----------------------------------
 * Lattice: a box lo[a] < hi[a] (finite) and n[a] >= 1 cubes per axis; spacing h[a] = (hi[a] - lo[a]) / n[a]; lattice point (i, j, k)
 * at x_i = lo[0] + (double)i * h[0] (two roundings, no fused multiply-add), the same for y and z; index L(i,j,k) = i + (n0+1) (j +
 * (n1+1) k), x fastest.  The value at a lattice point is hpsdf_query_device's at that point on the same context, bit for bit (the
 * lattice kernel runs Query's own device code).  (n0+1)(n1+1)(n2+1) <= 2^30, and both extreme lattice points (lo and lo + n h) must
 * pass Query's containment test, so that no value is DBL_MAX -- the root AABB itself passes; otherwise HPSDF_ERR_INVALID_ARGUMENT
 * and hpsdf_last_error() names the axis.
 * Classification: a corner is inside iff v < iso (strict; iso finite).  Case of cube (i,j,k): bit dx + 2 dy + 4 dz is set iff
 * corner (i+dx, j+dy, k+dz) is inside.
 * Vertices: one per lattice edge whose ends differ in insideness.  An edge runs from its lower point a to b = a + e_axis;
 * t = (iso - v_a) / (v_b - v_a); the coordinate along the axis is x_a + t (x_b - x_a), the other two are a's exactly; doubles.
 * Edge id 3 L(a) + axis; vertices are numbered in increasing edge id.
 * Triangles: ordered by cube Q = i + n0 (j + n1 k), then in case-table order within the cube; indices uint64_t; counter-clockwise
 * seen from the side where values are >= iso (normals point towards increasing value: outward for an SDF negative inside -- the
 * winding hpsdf_field_create_mesh expects).
 * Case table: generated by a face-local rule (csrc/surface_table.hpp).  Cube-local edges: x 0->1, 2->3, 4->5, 6->7 = 0..3;
 * y 0->2, 1->3, 4->6, 5->7 = 4..7; z 0->4, 1->5, 2->6, 3->7 = 8..11.  On each face the crossing edges are joined by segments: one
 * around an odd corner (1 or 3 inside), one for 2 adjacent inside corners, two for 2 diagonal inside corners (the inside corners
 * are separated).  The segments close into loops, each fan-triangulated from its first edge (listed from the smallest) whose
 * diagonals all leave the cube's faces.  Adjacent cubes agree on every shared face, so the
 * mesh is watertight and edge-manifold wherever the surface does not leave the box.  At most HPSDF_SURFACE_MAX_TRIS triangles a
 * case; row c of hpsdf_surface_case_table: 3 cube-local edges a triangle, then -1.  Host-only: needs no device. */
#define HPSDF_SURFACE_MAX_TRIS 5
HPSDF_API int hpsdf_surface_case_table(int8_t out[256 * 16]);
/* Host call, synchronous on the context stream.  *verts (3 doubles a vertex) and *tris (3 indices a triangle) are malloc'd; the
 * caller frees them.  An empty result is HPSDF_OK with counts 0 and NULL pointers.  values (may be NULL): every lattice value, L
 * order.  On any error nothing is allocated and the context stays usable; a failed allocation is HPSDF_ERR_OUT_OF_MEMORY.  Device
 * scratch: 8 bytes a lattice point for the values, ~1.1 more for the crossing bit words, their prefixes and the per-tile triangle
 * counts (under 10 bytes a point, plus a few KiB for the scans), then the outputs themselves (24 bytes a vertex and a triangle);
 * all of it is freed before the call returns. */
HPSDF_API int hpsdf_extract_surface(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3],
                                    double iso, double** verts, uint64_t* n_verts, uint64_t** tris, uint64_t* n_tris, double* values);
/* device milliseconds of the phases of this thread's last hpsdf_extract_surface: [0] lattice values, [1] classification and counts,
 * [2] scans, [3] vertex and triangle output, [4] download, [5] the whole call from its first launch (events on the context stream) */
HPSDF_API int hpsdf_surface_last_timings(double ms[6]);

/* ---- sparse ExtractSurface: the same mesh, evaluated only where the tree cannot rule the surface out --------------------------------
 * Same geometry as hpsdf_extract_surface: the lattice, the point arithmetic lo + (double)i * h, the classification v < iso, the vertex
 * arithmetic, the case table, the edge ids 3 L + axis, vertices in increasing edge id, triangles by cube Q then in case-table order,
 * the winding, malloc'd outputs and the empty result (HPSDF_OK, counts 0, NULL pointers).  For any arguments the dense call accepts
 * the sparse call returns bitwise the same verts and tris.  There is no values output; the limits are (n0+1)(n1+1)(n2+1) <= 2^40 and
 * n[a] <= 2^20 (edge ids and cube keys then fit 43 bits); the containment requirement on the two extreme lattice points is the dense
 * call's.  Failures as there: nothing stays allocated, the context stays usable, HPSDF_ERR_INVALID_ARGUMENT or
 * HPSDF_ERR_OUT_OF_MEMORY.
 * Blocks: HPSDF_SURFACE_BLOCK cubes per axis; block (bx, by, bz) covers cubes [8 b, min(8 b + 8, n)) per axis, its closed point range
 * is one point wider on the upper side; block index bx + nb0 (by + nb1 bz), nb[a] = ceil(n[a] / 8).
 * Block classes: 0 must be evaluated; 1 every lattice point of the closed range has v >= iso; 2 every one has v < iso.  1 and 2 are
 * given only when proven, by this bound.  A leaf of degree p at depth d is f(u) = sum_r c_r prod_b nl[k_b(r)][d] P_{k_b(r)}(u_b) in
 * its unit coordinates u (P_k: Legendre).  On [-1, 1], |P_k| <= 1 and |P_k'| <= k (k + 1) / 2, so with
 *     G_a = sum_r |c_r| prod_b nl[k_b(r)][d] k_a(r) (k_a(r) + 1) / 2        and        S = sum_r |c_r| prod_b nl[k_b(r)][d]
 * every u of a box of half-extents rho_a around u_c has |f(u) - f(u_c)| <= sum_a rho_a G_a (mean value theorem along the segment).
 * One lane per block walks the tree from the root with the block's two extreme lattice points pushed through Query's own
 * expressions p = (x - rootCentre) * rootInvSizes and "p >= centre" -- monotone per axis, so on an axis the lower child is visited if
 * p_lo < c and the upper one if p_hi >= c: a superset of the leaves any lattice point of the block reaches.  In each visited leaf the
 * block's range in unit coordinates (again Query's expression (p - centre) * (2 << depth) on the extreme points, monotone too) is
 * clipped to [-(1 + E), 1 + E], f_c is the leaf's polynomial at the clipped box's centre (the leaf evaluation Query uses) and the
 * leaf passes if
 *     |f_c - iso| > HPSDF_SURFACE_SLACK * sum_a rho_a G_a + HPSDF_SURFACE_ETA * S.
 * The block is class 1 (2) if every visited leaf passes with f_c > iso (< iso); class 0 if a leaf fails, the signs differ, more than
 * HPSDF_SURFACE_MAX_LEAVES leaves are visited or a corner fails the containment test.
 * The slack, derived (not tuned).  E = 2^-14: the f32 containment test admits p up to 0.5 + 2^-25 (half an f32 ulp above 0.5), which
 * the deepest leaf (depth 10, scale 2^11) sees as |u| <= 1 + 2^-14; inside the root Query's comparisons keep |u| <= 1.  A polynomial
 * of degree k bounded by M on [-1, 1] is bounded by M T_k(x) at |x| > 1 (Chebyshev's extremal property), so on [-(1 + E), 1 + E]
 * |P_k| <= tau and |P_k'| <= tau k (k + 1) / 2 with tau = T_12(1 + 2^-14) = cosh(12 acosh(1 + 2^-14)) < 1.0089.  Every term of
 * df/du_a is one derivative times two values: sup |df/du_a| <= tau^3 G_a < 1.0268 G_a.  HPSDF_SURFACE_SLACK = 1 + 2^-5 = 1.03125
 * covers that and leaves 0.4 % for the roundings of G_a (455 positive terms), of the centre and of the half-extents (a few ulps
 * each).  HPSDF_SURFACE_ETA = 2^-32 covers the difference between the computed and the exact polynomial at the lattice points and
 * at the centre: the recurrence to degree 12 and the three-factor products err by less than 2^11 ulps of a term, the sum of up to
 * 455 terms by 2^9 more, both relative to tau^3 S -- under 2^-41 S an evaluation, 2^-40 S for the two; 2^-32 is 2^8 above that.
 * Device scratch: one class byte per block, 40 bytes per tree node for the constants, 8 + 8 bytes per active block and its two
 * prefixes, 80 bytes a vertex and 88 a triangle while they are sorted (keys, indices and their sorted copies, records, outputs) plus
 * rocPRIM's temporaries -- nothing else grows with the lattice's volume (the dense call: under 10 bytes a lattice point).  All of it
 * is freed before the call returns; stats->peak_scratch_bytes is the most the call held at once, outputs included. */
#define HPSDF_SURFACE_BLOCK 8
#define HPSDF_SURFACE_MAX_LEAVES 64
#define HPSDF_SURFACE_SLACK 1.03125              /* 1 + 2^-5 */
#define HPSDF_SURFACE_ETA 2.3283064365386963e-10 /* 2^-32 */
typedef struct hpsdf_surface_sparse_stats { /* 96 bytes */
    uint64_t blocks, active_blocks; /* all blocks; blocks of class 0 */
    uint64_t leaves_visited;        /* by the classification, summed over the blocks */
    double classify_ms, count_ms, scan_ms, emit_ms, sort_ms, download_ms, total_ms; /* device milliseconds: constants and classes;
                                       per-block counts; compaction and prefix scans; records; sorts, renumbering and gathers; copies
                                       to the host; the whole call from its first launch */
    uint64_t peak_scratch_bytes;
    uint64_t reserved;
} hpsdf_surface_sparse_stats;
HPSDF_API int hpsdf_extract_surface_sparse(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3],
                                           const uint32_t n[3], double iso, double** verts, uint64_t* n_verts, uint64_t** tris,
                                           uint64_t* n_tris, hpsdf_surface_sparse_stats* stats /* may be NULL */);
/* Diagnostics: the class byte of blocks [first_block, first_block + count) into out (host memory).  _host works from a serialised block
 * on the calling thread (no device) with the kernel's statements: the same bytes as _device. */
HPSDF_API int hpsdf_surface_classify_host(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3],
                                          double iso, uint64_t first_block, uint64_t count, uint8_t* out);
HPSDF_API int hpsdf_surface_classify_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3],
                                            const uint32_t n[3], double iso, uint64_t first_block, uint64_t count, uint8_t* out);

/* ---- ExtractSurfaceDual: dual contouring over the same lattice -- one vertex a cube, placed by the field's tangent planes, so creases
 * and corners of the solid survive (no reference counterpart) ------------------------------------------------------------------------
 * Carried over from hpsdf_extract_surface unchanged: the lattice, its limits and checks ((n0+1)(n1+1)(n2+1) <= 2^30, the containment
 * requirement), the point arithmetic lo + (double)i * h, the lattice values, the classification v < iso, the cube cases, the edge ids
 * 3 L + axis, the cube order Q = i + n0 (j + n1 k), the cube-local edge numbering 0..11, malloc'd outputs the caller frees, and that
 * on any error nothing is allocated.  tau must be finite with 0 <= tau < 1 and flags must be 0; anything else is
 * HPSDF_ERR_INVALID_ARGUMENT.
 * Hermite sample, one per crossing edge e (an edge whose ends differ in insideness): p_e is hpsdf_extract_surface's vertex of that
 * edge, by the same statements with the same bits; (f_e, g_e) is QueryGradient (hpsdf_query_true_gradient_*, flags 0: not
 * normalised) at p_e on the same context, bit for bit.
 * Vertex: one per mixed cube (case neither 0 nor 255), numbered in increasing Q.  With the cube's k crossing edges taken in
 * cube-local order 0..11, every statement rounded once, no fused multiply-add, sums started from 0.0:
 *     s = sum_e p_e (per axis, in that order),  m = s / (double)k,  d_e = p_e - m,
 *     r_e = (iso - f_e) + sum3(g_e0 d_e0, g_e1 d_e1, g_e2 d_e2)      sum3(a, b, c) = a + (b + c), or (a + b) + c under reduction
 *                                                                     order 1 (the context's; as in CastRays),
 *     A_ij = A_ij + g_ei g_ej (all nine, so A stays symmetric),  b_i = b_i + g_ei r_e       in edge order.
 * A is decomposed by cyclic Jacobi: V = I, then HPSDF_DUAL_SWEEPS sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third
 * index.  A rotation is skipped when A_pq is exactly 0; otherwise
 *     theta = (A_qq - A_pp) / (2.0 * A_pq),   t = 1.0 / (|theta| + sqrt(theta * theta + 1.0)),  negated if theta < 0,
 *     c = 1.0 / sqrt(t * t + 1.0),  s = t * c,
 *     A_pp = A_pp - t * A_pq,  A_qq = A_qq + t * A_pq,  A_pq = A_qp = 0,
 *     (A_rp, A_rq) = (c * A_rp - s * A_rq,  s * A_rp + c * A_rq)  from the old pair, mirrored into A_pr, A_qr,
 *     (V_kp, V_kq) = (c * V_kp - s * V_kq,  s * V_kp + c * V_kq)  for k = 0, 1, 2.
 * The number of sweeps is fixed; there is no data-dependent loop.  lambda_i = A_ii, v_i = column i of V, lambda_max the largest of
 * the three.  Starting from x = m, for i = 0, 1, 2 with lambda_i > tau * lambda_max and lambda_i > 0:
 *     w = sum3(V_0i b_0, V_1i b_1, V_2i b_2) / lambda_i,   x_a = x_a + V_ai * w,
 * the rank being the number of such i.  If lambda_max is not positive or not finite, or a coordinate of x is not finite, x = m and
 * the rank is 0 (a cube whose samples all lie in leaves of degree 0 has A = 0).  Then x_a is clamped into [X_a(i_a), X_a(i_a + 1)],
 * the lattice coordinates lo[a] + (double)i * h[a] of the cube's corner points.  vert_info[v]: the rank in bits 0-1,
 * HPSDF_DUAL_CLAMPED if an axis was clamped.
 * Sweeps: HPSDF_DUAL_SWEEPS = 5, chosen so that after the last sweep the largest |off-diagonal| entry is at most 2^-40 of the trace.
 * Measured through the _block entry over every cube of tests/test_surface_dual_cpu.py (87 273 of them; test_jacobi_sweeps_suffice):
 * 2.6e-101 of the trace after 5 sweeps, 1.1e-24 after 4, 1.2e-6 after 3 -- cyclic Jacobi converges quadratically.
 * Triangles: a crossing edge along axis a at lattice point (i, j, k) is interior when its indices on the other two axes
 * b = (a + 1) % 3 and c = (a + 2) % 3 lie in [1, n - 1].  An interior crossing edge gives one quad over the vertices of the four
 * cubes at (b, c) offsets (-1,-1), (0,-1), (0,0), (-1,0) from (i, j, k) -- q0 q1 q2 q3, counter-clockwise seen from +a -- taken as
 * q0 q3 q2 q1 when the edge's lower end is outside (v >= iso), and split as (q0, q1, q2), (q0, q2, q3).  Triangles are ordered by
 * edge id, two per interior crossing edge; normals point towards increasing value, as with marching cubes.  Crossing edges on the
 * lattice's boundary give nothing: the mesh is open where the surface leaves the box.
 * Results: the vertices are returned whenever there is a mixed cube, even without a triangle; an empty result is HPSDF_OK with
 * counts 0 and NULL pointers.  vert_info (may be NULL): *vert_info is a malloc'd byte a vertex (NULL without vertices).  values (may
 * be NULL): every lattice value, L order.
 * Limits: one vertex a cube means that a cube face with four crossing edges (an ambiguous face) makes a non-manifold edge between
 * the two cubes' vertices.  The mesh is always closed where the surface stays inside the lattice (every directed edge has its
 * reverse, counted with multiplicity); it is edge-manifold where no face is ambiguous.
 * Device scratch: 8 bytes a lattice point for the values, ~1.6 more for the three bit words (crossing edges, interior crossing
 * edges, mixed cubes), their counts and prefixes, then 64 bytes a crossing edge (the Hermite record), 4 + 25 a mixed cube (the list,
 * the vertex and its info byte) and 24 a triangle; all of it is freed before the call returns.
 * _block: the same statements on the calling thread from a serialised block -- no device, the process-wide reduction order, blocks
 * accepted and refused as by hpsdf_project_block -- with the same bits in every output as the device call. */
#define HPSDF_DUAL_SWEEPS 5
#define HPSDF_DUAL_CLAMPED 4u
HPSDF_API int hpsdf_extract_surface_dual(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3],
                                         double iso, double tau, uint32_t flags, double** verts, uint64_t* n_verts, uint64_t** tris,
                                         uint64_t* n_tris, uint8_t** vert_info /* may be NULL */, double* values /* may be NULL */);
HPSDF_API int hpsdf_extract_surface_dual_block(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3],
                                               double iso, double tau, uint32_t flags, double** verts, uint64_t* n_verts, uint64_t** tris,
                                               uint64_t* n_tris, uint8_t** vert_info /* may be NULL */, double* values /* may be NULL */);
/* device milliseconds of the phases of this thread's last hpsdf_extract_surface_dual: [0] lattice values, [1] the three ballots and
 * their counts, [2] scans, [3] Hermite samples, [4] cube list and vertices, [5] quads, [6] download, [7] the whole call from its first
 * launch (events on the context stream) */
HPSDF_API int hpsdf_surface_dual_last_timings(double ms[8]);

/* ---- QueryBounds: a guaranteed range of Query over axis-aligned boxes (no reference counterpart) ---------------------------------------
 * One row per box: six doubles, the lower corner a[3] then the upper corner b[3], world coordinates.  The result is an interval
 * [lo, hi] with this guarantee: for every point x with a <= x <= b componentwise, Query(x) -- the double this library computes at x,
 * not the polynomial's exact value -- satisfies lo <= Query(x) <= hi.  A sampled minimum proves nothing about a region; this does,
 * because a leaf is a polynomial whose variation over a box is bounded by its coefficients.  The rule is the block classification's
 * (hpsdf_extract_surface_sparse above: G_a, S, E, the child selection, HPSDF_SURFACE_SLACK, HPSDF_SURFACE_ETA), with the block of
 * cubes replaced by any box and the class byte by the interval.  Host, device and block entries run the same statements
 * (csrc/tree_bound.hpp, boundsWalk; every expression below has the association written, no multiply-add is fused) and give the same
 * bits.  Per call: subdiv in {1, 2, 4}, max_leaves in 1..65535.
 *   1 map      pl_a = (a_a - rootCentre_a) * rootInvSizes_a,  ph_a = (b_a - rootCentre_a) * rootInvSizes_a: Query's own expression on the
 *              two extreme points.  If (float)pl_a or (float)ph_a is outside [-0.5, 0.5] on an axis (Query's containment test; a NaN
 *              or infinite coordinate fails it) or !(pl_a <= ph_a):       status = HPSDF_BOUNDS_INVALID, lo = hi = quiet NaN, leaves = 0
 *   2 walk     lo = +inf, hi = -inf, leaves = 0.  From the root, depth first, the children of a node centred at c in increasing
 *              index, child i visited iff on every axis (bit a of i clear and pl_a < c_a) or (bit a of i set and ph_a >= c_a): Query
 *              takes the upper child iff p_a >= c_a and p is monotone in x, so this is a superset of the leaves any point of the box
 *              reaches.  Centres are exact dyadics.  At each leaf reached:
 *                if leaves == max_leaves:                          status = HPSDF_BOUNDS_LEAF_LIMIT, lo = -inf, hi = +inf, stop
 *                leaves = leaves + 1
 *   3 bound    in that leaf (depth d, centre c, s = 2^(d+1)), per axis:  ua = (pl_a - c_a) * s,  ub = (ph_a - c_a) * s  (Query's
 *              expression, monotone too);  if ua < -(1 + E): ua = -(1 + E);  if ub > 1 + E: ub = 1 + E  (E = 2^-14);  if !(ua <= ub)
 *              on an axis no point of the box lies in the leaf: next leaf.  Otherwise w_a = (ub - ua) * (1.0 / subdiv), and for the
 *              subdiv^3 sub-boxes (i, j, k), x fastest, then y, then z, per axis with its index m:
 *                l = ua + (double)m * w_a;   h = (m + 1 == subdiv) ? ub : ua + (double)(m + 1) * w_a
 *                u_c = 0.5 * (l + h);   rho = 0.5 * (h - l)
 *              (h of one sub-box and l of the next are the same expression: the sub-boxes tile [ua, ub] exactly), then
 *                f_c = the leaf's polynomial at u_c, by the leaf evaluation Query uses
 *                e   = HPSDF_SURFACE_SLACK * ((rho_0 * G_0 + rho_1 * G_1) + rho_2 * G_2) + HPSDF_SURFACE_ETA * S
 *                if f_c or e is not finite:                        status = HPSDF_BOUNDS_NOT_FINITE, lo = -inf, hi = +inf, stop
 *                el = f_c - e and eh = f_c + e, each rounded TOWARDS f_c: the smallest double >= the exact f_c - e, the largest double <=
 *                the exact f_c + e (the rounded sum, or its neighbour on f_c's side where the sum rounded away from f_c; the rounding
 *                error of an addition is a double and is computed exactly, so this too is the same bits everywhere)
 *                if (el < lo) lo = el;      if (eh > hi) hi = eh
 *   4 result   status = HPSDF_BOUNDS_OK with [lo, hi] (a valid box reaches at least one leaf, so lo <= hi), leaves = the leaves passed.
 * The infinite intervals of LEAF_LIMIT and NOT_FINITE are true statements, not errors; `leaves` then holds the count at the stop
 * (max_leaves for LEAF_LIMIT).  subdiv = 1 bounds a leaf's part of the box as the block classification does; 2 and 4 halve and
 * quarter rho per axis at 8 and 64 evaluations a leaf: e shrinks roughly in proportion until HPSDF_SURFACE_ETA * S, the floor of a
 * point box, is what is left.
 * Why it holds, and why the classification's constants still cover this use (derived, not tuned; nothing was widened).
 *   Reach: a point x of the box has p(x) in [pl, ph] per axis (one subtraction and one multiplication by a positive number, both
 *   monotone), so the leaf Query descends to is visited, and there its u lies in [ua, ub] before clipping and, by the containment
 *   test, within [-(1 + E), 1 + E]: in exactly one sub-box's [l, h] up to the shared faces.
 *   Variation: with u_c and rho exact, |f(u) - f(u_c)| <= tau^3 sum_a rho_a G_a, tau^3 < 1.0268 (the sparse section's argument; it
 *   never used the block's shape).  subdiv only shrinks rho, which the mean value bound is linear in, and changes nothing else.
 *   Relative roundings: G_a (455 positive terms: under 2^-43 relative), rho (one subtraction), the three products and two sums of e
 *   and the multiplication by the slack are each a few ulps relative; 1.03125 / 1.0268 leaves 0.4 % for them, as before.
 *   The one rounding that is NOT relative to rho: u_c = 0.5 * (l + h) is off by up to 2^-53 (half an ulp below 2), which moves the
 *   centre by that much whatever rho is -- a box a few ulps wide has its centre on one of its ends.  The classification has the same
 *   term (its blocks are never that thin, but nothing forbids it).  It is absolute, so it is charged to ETA: sup |df/du_a| <= tau^3
 *   G_a and G_a <= 78 S (k (k + 1) / 2 <= 78 for k <= 12), hence at most 3 * 2^-53 * 78 * 1.0268 S < 2^-45 S over the three axes.
 *   Evaluation: Query(x) and f_c each differ from the exact polynomial by under 2^-41 S (the sparse section): 2^-40 S for the two.
 *   f_c -/+ e: the two ends are rounded towards f_c, which takes less than one spacing of doubles off e: under 2^-52 (|f_c| + e) <=
 *   2^-52 (1.0268 S + e) -- 2^-51.9 S absolute plus a 2^-52 relative part of e that the 0.4 % takes.  Rounding to nearest would be as
 *   sound; towards f_c the interval is never wider than the rule's own 2 e: hi - lo <= 2 e in exact arithmetic, for every box.
 *   Sum charged to ETA: 2^-40 + 2^-45 + 2^-51.9 < 2^-39.9 S, against HPSDF_SURFACE_ETA = 2^-32: the 2^8 of headroom the sparse
 *   section left is now 2^7.9.  Both constants stay as they are.
 *   Not finite: a leaf with an infinite or NaN coefficient has S (and e) infinite or NaN and is reported as NOT_FINITE, never bounded.
 *   A point box (a == b): every sub-box is the point, f_c is Query(a) bit for bit, e is ETA S with one rounding, and lo <= Query(a) <= hi
 *   with hi - lo <= 2 ETA S (1 + 2^-43): the ends' rounding adds nothing to the width.
 * Outputs per box: out_lo, out_hi (double) and out_status (uint8_t, HPSDF_BOUNDS_*) are required; out_leaves (uint32_t) is optional:
 * when NULL it takes no slot and is left untouched.
 * hpsdf_query_bounds_grid_*: the boxes are the cells of a lattice lo[3], hi[3], n[3] (hpsdf_extract_surface's arguments and checks:
 * finite, lo < hi, n >= 1, both extreme points inside the root), h_a = (hi_a - lo_a) / n_a; box i + n0 (j + n1 k) is cell (i, j, k)
 * with corners lo_a + (double)i * h_a and lo_a + (double)(i + 1) * h_a -- the surface lattice's own arithmetic, so neighbouring cells
 * share their faces exactly; n0 n1 n2 <= 2^32.  No box array is materialised; the outputs hold n0 n1 n2 rows, x fastest, and are the
 * box entries' bits for the same corners.
 * A NULL tree, a required array NULL with n > 0 (grid: NULL lo, hi or n), subdiv not 1, 2 or 4, max_leaves outside 1..65535, a
 * lattice hpsdf_extract_surface would refuse: HPSDF_ERR_INVALID_ARGUMENT, and no output is written.  n == 0 is HPSDF_OK.  _device is
 * asynchronous on the context stream, except that the first bounds call on a tree builds the leaves' constants G_a, S once, under a
 * lock, on the context stream, and WAITS for that stream on the host before it launches (a call on another stream must find them
 * complete); it keeps them with the tree until hpsdf_tree_destroy: 32 bytes a node; every later call only launches; _host answers calls of up to 32
 * boxes on the calling thread and sends larger ones through the device; _block needs no device: it works from a serialised block on
 * the calling thread and accepts and refuses blocks as hpsdf_project_block does.
 * Not done: boxes reaching outside the root are INVALID, not clipped; a large box is one lane's walk (see max_leaves); the enclosure
 * is first order (it does not use the gradient at the centre). */
enum { HPSDF_BOUNDS_OK = 0, HPSDF_BOUNDS_LEAF_LIMIT = 1, HPSDF_BOUNDS_INVALID = 2, HPSDF_BOUNDS_NOT_FINITE = 3 };
HPSDF_API int hpsdf_query_bounds_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* d_boxes, size_t n, uint32_t subdiv,
                                        uint32_t max_leaves, double* d_out_lo, double* d_out_hi, uint8_t* d_out_status,
                                        uint32_t* d_out_leaves);
HPSDF_API int hpsdf_query_bounds_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* boxes, size_t n, uint32_t subdiv, uint32_t max_leaves,
                                      double* out_lo, double* out_hi, uint8_t* out_status, uint32_t* out_leaves);
HPSDF_API int hpsdf_query_bounds_block(const void* block, size_t size, const double* boxes, size_t n, uint32_t subdiv, uint32_t max_leaves,
                                       double* out_lo, double* out_hi, uint8_t* out_status, uint32_t* out_leaves);
HPSDF_API int hpsdf_query_bounds_grid_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3],
                                             uint32_t subdiv, uint32_t max_leaves, double* d_out_lo, double* d_out_hi, uint8_t* d_out_status,
                                             uint32_t* d_out_leaves);
HPSDF_API int hpsdf_query_bounds_grid_host(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3],
                                           uint32_t subdiv, uint32_t max_leaves, double* out_lo, double* out_hi, uint8_t* out_status,
                                           uint32_t* out_leaves);
HPSDF_API int hpsdf_query_bounds_grid_block(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3],
                                            uint32_t subdiv, uint32_t max_leaves, double* out_lo, double* out_hi, uint8_t* out_status,
                                            uint32_t* out_leaves);

/* ---- Integrate: volume bounds and moments of the solid {x in root : Query(x) < iso} (no reference counterpart) --------------------------
 * The integral counterpart of QueryBounds: the leaves of the tree are refined level by level into dyadic cells, a cell's sign is decided
 * by QueryBounds' rule at ONE evaluation of its leaf's polynomial, and only the cells the rule cannot decide -- those the surface passes
 * through -- are split.  The work grows with the surface's area (4^depth), not with the root's volume (8^depth).  The result is
 *   - a guaranteed enclosure  volume_lo <= vol{x in root : Query(x) < iso} <= volume_hi  (in the sense of QueryBounds: Query(x) is the
 *     double this library computes; see "Why it holds" below),
 *   - an estimate of the zeroth, first and second moments of that solid: volume, the integral of x (3 numbers) and of x x^T (6 numbers
 *     in the order xx, yy, zz, xy, xz, yz),
 *   - optionally the final cells themselves: an adaptive voxelisation of the solid and of a narrow band around its surface.
 * The region is the whole root box.  Host, device and block entries run the same statements (csrc/integrate.hpp; every expression
 * below has its association written, no multiply-add is fused, -ffp-contract=off) and give the same bits.
 * Arguments: iso finite; depth D in 0..15; samples q in {1, 2, 4}; max_cells in 8..2^28.
 *   A cell     is a leaf node n (tree depth d) at a relative level l >= 0 with integer coordinates in [0, 2^l)^3 inside the leaf; its
 *              absolute depth is a = d + l.  In the leaf's unit coordinates, per axis with its coordinate m:
 *                lo = -1.0 + (double)m * w,  w = 2.0 / (double)(1 << l);   hi = lo + w;   u_c = 0.5 * (lo + hi);   rho = 1.0 / (double)(1 << l)
 *              -- all exact dyadics.  In the root's normalised frame p in [-0.5, 0.5]^3 its edge is s = 1.0 / (double)(1 << a) and, with
 *              (i, j, k) its integer coordinates at depth a (the leaf's own coordinates shifted left by l, plus m), per axis
 *                plo = -0.5 + (double)i * s;   c = plo + 0.5 * s                                         -- exact too.
 *   Class      f_c = the leaf's polynomial at u_c, by the leaf evaluation Query uses
 *              e   = HPSDF_SURFACE_SLACK * ((rho * G_0 + rho * G_1) + rho * G_2) + HPSDF_SURFACE_ETA * S
 *              1 (outside) if f_c - iso > e;  else 2 (inside) if iso - f_c > e;  else 0 (undecided).
 *              If f_c or e is not finite in any cell the whole call ends with status HPSDF_INTEGRATE_NOT_FINITE: unit_volume_lo = 0,
 *              unit_volume_hi = 1 (volume_lo = 0, volume_hi = J), every estimate a quiet NaN, the counts 0, no cells.
 *   Lists      List 0 holds the leaves in increasing node index, each at l = 0.  List l + 1 holds, for every cell of list l that is
 *              undecided with a < D, in list order, its 8 children in child index order (x fastest: child ch has coordinates
 *              2 i + (ch & 1), 2 j + ((ch >> 1) & 1), 2 k + (ch >> 2) at depth a + 1).  Positions in the next list come from an
 *              exclusive scan of the split flags; no atomic decides an order.  If the next list would hold more than max_cells cells,
 *              no cell of this level is split: the level is final and the status is HPSDF_INTEGRATE_CELL_LIMIT -- the result degrades
 *              (a wider enclosure), it does not fail.  `levels` is l of the last list.
 *   Final      A final cell is a decided cell at any level, or an undecided cell that is not split.  With v = (s * s) * s and the box
 *              moments of a box of edge s, volume v and centre c
 *                M0 = v;   M1_k = v * c_k;   M2_kk = v * (c_k * c_k + (s * s) / 12.0);   M2_jk = v * (c_j * c_k)
 *              an inside cell adds v to unit_volume_lo and its box moments to the estimate; an outside cell adds nothing; an undecided
 *              cell adds v to unit_volume_hi - unit_volume_lo and, for the estimate, takes its q^3 sub-boxes of edge ss = s * (1.0 / q),
 *              x fastest, then y, then z: sub-box m per axis has its centre at u = lo + (double)(2 m + 1) * ((0.5 * w) * (1.0 / q)) in
 *              the leaf and at p = plo + (double)(2 m + 1) * (0.5 * ss) in the root's frame (exact); the polynomial is evaluated at u,
 *              and a sub-box with value < iso adds its box moments (edge ss, volume (ss * ss) * ss, centre p) to the cell's row, in
 *              sub-box order, row = row + moments.
 *   Sums       Volumes are exact: with D <= 15 and q <= 4 every volume term is a multiple of 2^-51 (a leaf is never deeper than
 *              HPSDF_TREE_MAX_DEPTH), and every partial sum is at most 1, so no addition of volumes rounds and their order cannot
 *              matter; unit_volume_lo, unit_volume_hi and unit_volume are exact rationals and unit_volume_lo <= unit_volume <=
 *              unit_volume_hi holds exactly.  The cell counts are integers below 2^53 and go the same way.  First and second moments
 *              are not exact; their sum is DEFINED: the rows of a list's cells (a split cell's row is zero) are taken in list order in
 *              blocks of 256, zero-padded; lane t holds row t; for stride = 128, 64, ..., 1: x[t] = x[t] + x[t + stride] for t <
 *              stride; the block sums are reduced by the same rule until one row is left; the level totals are added in increasing
 *              l, ((T0 + T1) + T2) ...  The kernel keeps a cell's row in registers and writes one row per workgroup.
 *   World      x_k = rootCentre_k + p_k * size_k with size_k = 1.0 / rootInvSizes_k and J = (size_0 * size_1) * size_2:
 *                volume_lo = J * unit_volume_lo;   volume_hi = J * unit_volume_hi;   volume = J * M0
 *                m1_k  = J * (rootCentre_k * M0 + size_k * M1_k)
 *                m2_jk = J * (((rootCentre_j * rootCentre_k) * M0 + (rootCentre_j * size_k) * M1_k)
 *                             + ((rootCentre_k * size_j) * M1_j + (size_j * size_k) * M2_jk))
 *              computed on the host from the normalised sums (these four roundings are outside the guarantee: the guaranteed pair
 *              is unit_volume_lo, unit_volume_hi).
 * Why it holds, and why the existing constants cover this use (nothing was retuned).  The variation bound |f(u) - f(u_c)| <= tau^3
 * sum_a rho_a G_a and the evaluation error 2^-41 S are QueryBounds' (above), with u_c and rho exact here -- the cell is GIVEN in unit
 * coordinates, not mapped from world corners, so the 2^-45 S centre term does not even arise.  What replaces it: a point x of the cell
 * reaches the leaf with u computed by Query from x through two subtractions and two multiplications, which may fall a few ulps (of
 * 2, the unit cube's size: under 2^-50) outside [lo, hi]; sup |df/du_a| <= tau^3 G_a and G_a <= 78 S, so f moves by under 78 * 1.0268 *
 * S * 2^-50 < 2^-43.6 S per axis, charged to ETA: 2^-40 + 3 * 2^-43.6 < 2^-39.6 S against ETA = 2^-32 S.  The comparison's left side
 * f_c - iso is one rounding, relative 2^-53 of the very quantity compared with e, which the 0.4 % that SLACK leaves over tau^3
 * takes.  The same rounding of x can carry a point within 2^-52 (relative) of a leaf's face into the neighbouring leaf, where another
 * polynomial answers; these points form shells of relative thickness 2^-52 around leaf faces, and the enclosure is of the solid in
 * the root's frame p, up to that measure.
 * Outputs: hpsdf_integral (below); optionally *out_cells, a malloc'd array of the final cells (hpsdf_extract_surface's convention: the
 * caller frees it; an empty result is NULL with *out_n_cells = 0; pass out_cells = out_n_cells = NULL to get none), in list order,
 * level by level, 12 bytes a cell: the cell is [-0.5 + i * 2^-depth, -0.5 + (i + 1) * 2^-depth) x ... in p.  Over all final cells the
 * volumes 8^-depth sum to 1: they tile the root.
 * iso not finite, depth > 15, samples not 1, 2 or 4, max_cells outside 8..2^28, a NULL tree or `out`, only one of out_cells and
 * out_n_cells NULL: HPSDF_ERR_INVALID_ARGUMENT, and nothing is written.  On any failure nothing stays allocated and the context stays
 * usable.  hpsdf_integrate_device runs on the context stream (one classify kernel, one rocPRIM scan, one contribute kernel and the
 * row reduction per level) and synchronises before it returns; list 0 and the leaves' constants are made by the first call on a tree and
 * kept with it until hpsdf_tree_destroy.  hpsdf_integrate_host computes on the calling thread from the tree's host copies (fetched
 * once), hpsdf_integrate_block from a serialised block with no device at all; it accepts and refuses blocks as
 * hpsdf_query_bounds_block does.
 * Not done: regions other than the root (no clipping to a sub-box); surface area; a linear reconstruction in the finest cells (the
 * estimate is a q^3-point sign count there: first order in s it is not); rigorous bounds on the first and second moments beyond what
 * |p_k| <= 0.5 gives from the undecided volume U = unit_volume_hi - unit_volume_lo (the true M1_k lies within U / 2 of the inside
 * cells' sum, M2_kk within U / 4, M2_jk within U / 4). */
enum { HPSDF_INTEGRATE_OK = 0, HPSDF_INTEGRATE_CELL_LIMIT = 1, HPSDF_INTEGRATE_NOT_FINITE = 2 };
typedef struct hpsdf_integral {
    double unit_volume_lo, unit_volume_hi, unit_volume; /* root-normalised, exact */
    double volume_lo, volume_hi, volume;                /* world frame */
    double m1[3], m2[6];                                /* world frame: the integrals of x and of xx, yy, zz, xy, xz, yz */
    double unit_m1[3], unit_m2[6];                      /* the same in p */
    uint64_t cells_inside, cells_outside, cells_undecided; /* final cells by class */
    uint64_t evaluations;                               /* polynomial evaluations: the cells of all lists + q^3 per undecided final cell */
    uint32_t status;                                    /* HPSDF_INTEGRATE_* */
    uint32_t levels;                                    /* relative level of the last list */
} hpsdf_integral;
typedef struct hpsdf_integrate_cell {
    uint32_t node;    /* the leaf's node index */
    uint8_t depth;    /* absolute depth a */
    uint8_t cls;      /* 0 undecided, 1 outside, 2 inside */
    uint16_t i, j, k; /* integer coordinates at depth a */
} hpsdf_integrate_cell;
HPSDF_API int hpsdf_integrate_device(hpsdf_ctx* ctx, const hpsdf_tree* t, double iso, uint32_t depth, uint32_t samples, uint32_t max_cells,
                                     hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_integrate_host(hpsdf_ctx* ctx, const hpsdf_tree* t, double iso, uint32_t depth, uint32_t samples, uint32_t max_cells,
                                   hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_integrate_block(const void* block, size_t size, double iso, uint32_t depth, uint32_t samples, uint32_t max_cells,
                                    hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);

/* ---- IntegratePair: guaranteed volume of the CSG of two posed trees (no reference counterpart) ------------------------------------------
 * Integrate over tree A, with every cell also classified against a second tree B placed under an affine pose: the volume and moments of
 * the intersection, the union or the difference of the two solids, with no third tree built and no fit error added.
 *   SA = {x in A's root : Query_A(x) < iso_a}
 *   SB = {x : Query_B(M x + t) < iso_b}      (Query_B is DBL_MAX outside B's root: such points are not in SB)
 *   HPSDF_PAIR_INTERSECTION: SA n SB;   HPSDF_PAIR_UNION: (SA u SB) n A's root;   HPSDF_PAIR_DIFFERENCE: SA \ SB
 * pose[12] is the row-major 3 x 4 matrix [M | t]: a point x of A's world frame is y = M x + t in B's world frame.  M need not be a
 * rotation; nothing below uses more than |M_jk|.  The region is A's root, the cells are A's cells (hpsdf_integrate_cell, node an index
 * into A) and every result is in A's frame.  The output is hpsdf_integral with Integrate's meaning: unit_volume_lo <= vol(op) <=
 * unit_volume_hi is guaranteed (in Integrate's sense), volume, m1 and m2 are estimates; `evaluations` counts evaluations of A's
 * polynomial as Integrate does (the cells of all lists + q^3 per undecided final cell; work on B is not counted).  For the intersection
 * volume_hi == 0 proves the solids disjoint inside A's root and volume_lo > 0 proves that they interfere.
 * Arguments: iso_a, iso_b and the 12 pose entries finite; op <= 2; depth, samples, max_cells as in Integrate; max_leaves in 1..65535.
 * Host, device and block entries run the same statements (csrc/integrate_pair.hpp; every expression below has its association written,
 * no multiply-add is fused, -ffp-contract=off) and give the same bits.  The lists, the scan, the cell limit, the reduction, the level
 * totals and the world transform are Integrate's; only a cell's class and an undecided final cell's samples differ.
 *   Class of a cell
 *   1 clsA     Integrate's class of the cell on A with iso_a: one evaluation at the cell's centre.  (Not finite: as Integrate.)
 *   2 alone    intersection and difference: clsA outside -> outside; union: clsA inside -> inside.  B is not touched.
 *   3 box      otherwise the cell's image box [a, b] in B's world frame.  With s = 1.0 / (double)(1 << depth), size_k = 1.0 /
 *              rootInvSizesA_k and per axis k with its integer coordinate i:
 *                pc = (-0.5 + (double)i * s) + 0.5 * s          (exact)
 *                cx_k = rootCentreA_k + pc * size_k;   hx_k = (0.5 * s) * size_k
 *              and per row j of the pose:
 *                yc_j = ((M_j0 * cx_0 + M_j1 * cx_1) + M_j2 * cx_2) + t_j
 *                r_j  = (|M_j0| * hx_0 + |M_j1| * hx_1) + |M_j2| * hx_2
 *                a_j = yc_j - (r_j + delta_j);   b_j = yc_j + (r_j + delta_j)
 *              with the slack, one value a row for the whole call, computed once on the host,
 *                X_k = |rootCentreA_k| + 0.5 * size_k
 *                delta_j = (32 * 2^-53) * (((|M_j0| * X_0 + |M_j1| * X_1) + |M_j2| * X_2) + |t_j|)
 *   4 clamp    pl_k = (a_k - rootCentreB_k) * rootInvSizesB_k,  ph_k = (b_k - rootCentreB_k) * rootInvSizesB_k: Query's own expression
 *              (QueryBounds step 1).  PMAX = 0.5 + 2^-25 is the largest double whose (float) cast still passes Query's containment
 *              test (the cast rounds to nearest, ties to even, and 0.5f is even); PMIN = -PMAX.
 *                a NaN in pl or ph:                                         clsB undecided, no walk
 *                else (float)ph_k < -0.5f or (float)pl_k > 0.5f on an axis:   clsB outside, no walk (no point of the box reaches B)
 *                else if !((float)pl_k >= -0.5f): pl_k = PMIN, partial;      if !((float)ph_k <= 0.5f): ph_k = PMAX, partial
 *   5 walk     QueryBounds' steps 2 to 4 on B from [pl, ph] with subdiv = 1 and max_leaves: [lo, hi] and a status.
 *                clsB outside if lo > iso_b;  else inside if hi < iso_b and not partial;  else undecided
 *              HPSDF_BOUNDS_LEAF_LIMIT has [-inf, inf] and is therefore undecided.  HPSDF_BOUNDS_NOT_FINITE ends the call as a cell of A
 *              that is not finite does: status HPSDF_INTEGRATE_NOT_FINITE with Integrate's outputs.
 *   6 combine  operation      outside if                        inside if
 *              intersection   clsA or clsB is outside           both are inside
 *              union          both are outside                  clsA or clsB is inside
 *              difference     clsA is outside or clsB inside    clsA is inside and clsB outside
 *              everything else is undecided.
 *   A final undecided cell takes Integrate's q^3 sub-box centres u (in A's leaf) and p (in A's root frame).  At each:
 *                inA = f_A(u) < iso_a                                                       (Integrate's statements)
 *                x_k = rootCentreA_k + p_k * size_k;   y_j = ((M_j0 * x_0 + M_j1 * x_1) + M_j2 * x_2) + t_j
 *                inB = Query_B(y) < iso_b, by the point descent Query uses (DBL_MAX outside B's root and for a NaN)
 *              and the sub-box's moments are added iff the operation's predicate holds: inA && inB, inA || inB, inA && !inB.  (Where inA
 *              decides the predicate alone B is not asked; the value is the same.)
 * Why it holds.  A cell is decided only from statements true of every point of it: clsA is Integrate's; clsB outside means every point
 * of the image box either fails Query_B's containment test (value DBL_MAX, not < iso_b) or has Query_B > iso_b; clsB inside means
 * every point of the box passes the test (not partial) and has Query_B < iso_b; the table is the operation's predicate applied to
 * these.  What is left to show is that the box holds every y the statements above are about:
 *   the exact image, under the doubles M and t, of the cell's exact box {rootCentreA + p * size : p in the cell} -- the region the
 *   guarantee speaks of -- and every double y that step 6 computes from a p of the cell.
 *   Let u = 2^-53 and m_j = sum_k |M_jk| X_k + |t_j|; every point of A's root has |x_k| <= X_k, so m_j bounds the magnitudes that enter
 *   row j and |yc_j| + r_j <= m_j.  hx_k is exact (a power of two times size_k).  Roundings, each at most u times m_j to first order:
 *     cx_k (and x_k of step 6): one product and one sum, 2;  a row of M x + t: a product and up to three sums on the longest path, 4
 *     -- so yc_j is within 6 u m_j of the exact image of the exact centre, and a computed y within 6 u m_j of the exact image of its
 *     exact point;  r_j: a product and two sums, all positive, at most 3 u r_j too small;  r_j + delta_j: 1;  the last subtraction or
 *     addition: 1.
 *   An exact image lies within the exact r_j of the exact centre's image: 6 + 3 + 1 + 1 = 11.  A computed y adds its own 6: 17.  The
 *   second-order terms are below 17^2 u^2 m_j.  delta_j carries the constant 32: a headroom factor of 32 / 17 over the count.  It is
 *   derived, not tuned, and at 2^-48 of the scene's size it costs no cell its decision.  delta_j's own roundings (seven, all of positive
 *   terms) move it by under 2^-50 of itself.
 *   Steps 4 and 5: pl and ph are monotone in a and b (a subtraction and a multiplication by a positive number), so every y of the box
 *   has its p within [pl, ph] before the clamp; if (float)ph < -0.5f or (float)pl > 0.5f on an axis the cast of every such p fails the
 *   test, for the cast is monotone too.  A p the test passes lies in [PMIN, PMAX], so the clamped range still holds every point of the
 *   box that reaches B, and it passes QueryBounds' step 1: the walk's guarantee applies to it as it stands.
 *   An overflow in the chain gives an infinite end (clamped: partial) or a NaN (undecided): both only undecide.
 * Outputs, the cell array and its ownership are Integrate's.  A non-finite pose entry or iso, op > 2, a range outside those above, a
 * NULL tree, pose or `out`, only one of out_cells and out_n_cells NULL, two trees on different devices: HPSDF_ERR_INVALID_ARGUMENT,
 * and nothing is written.  tree_a == tree_b is allowed.  hpsdf_integrate_pair_device runs on the context stream (Integrate's launches
 * per level, with the pair kernels: a lane per cell, B walked with its stack in LDS) and synchronises before it returns; both trees'
 * constants and A's list 0 are the trees' own caches.  _host computes on the calling thread from the trees' host copies, _block from two
 * serialised blocks with no device at all; it accepts and refuses blocks as hpsdf_integrate_block does.
 * Not done: batches of poses in one call; subdiv above 1 on B; rigorous bounds on the moments (Integrate's remark applies); surface
 * area or contact normals; clipping the region to anything but A's root; a wave cooperating on one walk (a wave costs its slowest
 * lane, as in QueryBounds). */
enum { HPSDF_PAIR_INTERSECTION = 0, HPSDF_PAIR_UNION = 1, HPSDF_PAIR_DIFFERENCE = 2 };
HPSDF_API int hpsdf_integrate_pair_device(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, uint32_t op, const double pose[12],
                                          double iso_a, double iso_b, uint32_t depth, uint32_t samples, uint32_t max_cells, uint32_t max_leaves,
                                          hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_integrate_pair_host(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, uint32_t op, const double pose[12],
                                        double iso_a, double iso_b, uint32_t depth, uint32_t samples, uint32_t max_cells, uint32_t max_leaves,
                                        hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_integrate_pair_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, uint32_t op,
                                         const double pose[12], double iso_a, double iso_b, uint32_t depth, uint32_t samples, uint32_t max_cells,
                                         uint32_t max_leaves, hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);

/* ---- Clearance: guaranteed minimum of one tree's field over another's solid (no reference counterpart) --------------------------------
 * A branch-and-bound search over tree A's cells for
 *   m = inf { Query_B(M x + t) : x in A's root, Query_A(x) < iso_a, M x + t passes Query_B's containment test }
 * (a point whose image leaves B's root has the value DBL_MAX there and never lowers a minimum; m = +inf when no point qualifies).  It
 * returns an enclosure lo <= m <= hi and a witness point that attains hi.  When B is a distance field m - iso_b is the signed clearance
 * of solid A from solid B: positive, the solids are provably at least that far apart inside B's root; negative, it is the depth of A's
 * deepest point inside B and the witness is where that happens.  A tree against itself under the identity gives minus the radius of the
 * largest inscribed ball and its centre.  Only cells that can still hold the minimiser survive a level, so the work follows the contact
 * region and not the surface or the volume.  pose[12], the cells (Integrate's: hpsdf_integrate_cell, node an index into A), list 0 and
 * the child order are IntegratePair's and Integrate's.
 * Arguments: iso_a and the 12 pose entries finite; depth D in 0..15; tol finite and >= 0; max_cells in 8..2^28; max_leaves in 1..65535.
 * Host, device and block entries run the same statements (csrc/clearance.hpp; every association written, -ffp-contract=off) and give
 * the same bits.
 *   The rule.  best = +inf with no witness; finals is empty.  For each list l (the cells of relative level l, pos a cell's position in
 *   the list) three steps run in order:
 *   1 bound    clsA = Integrate's class of the cell on A with iso_a.  A cell that is not finite ends the call: status
 *              HPSDF_CLEARANCE_NOT_FINITE, lo = -inf, hi = +inf, point, image and value_a quiet NaNs, every counter 0, no cells.
 *              clsA outside: the cell is dropped and counted in cells_outside_a.  Otherwise IntegratePair's steps 3 and 4 (the image
 *              box with its slack delta, the clamp to B's root):
 *                no point of the box reaches B:  blo = +inf          a NaN:  blo = -inf
 *                else QueryBounds' walk of B over the clamped range with subdiv = 1 and max_leaves: blo = its lo (HPSDF_BOUNDS_LEAF_LIMIT
 *                gives -inf; HPSDF_BOUNDS_NOT_FINITE ends the call as above).
 *              Whether the box is partly outside B's root does not matter: such points cannot lower a minimum.
 *   2 witness  for every cell that was walked: x = cx, the cell's centre in A's world frame as IntegratePair's step 3 computes it;
 *              va = Query_A(x) by Query's point descent; if va < iso_a: y_j = ((M_j0 * x_0 + M_j1 * x_1) + M_j2 * x_2) + t_j and
 *              vb = Query_B(y); the cell is a candidate iff vb < DBL_MAX.  The level's candidate is the lexicographic minimum of
 *              (vb, pos) -- it does not depend on the order of evaluation -- and replaces best iff vb < best, strictly.
 *   3 prune    with the updated best a cell survives iff blo <= best and blo < +inf (a cell with blo = +inf holds no point with a value
 *              in B); the rest are counted in cells_pruned.  A survivor at absolute depth D is final and joins finals with its blo, a
 *              survivor above D is a split candidate.  L = min(blo of finals, blo of the split candidates).
 *              no finals and no split candidates:   status HPSDF_CLEARANCE_EMPTY, lo = hi = +inf, no witness, stop
 *              best - L <= tol:                     status HPSDF_CLEARANCE_CONVERGED, the split candidates join finals, stop
 *              8 * candidates > max_cells:          status HPSDF_CLEARANCE_CELL_LIMIT, the same, stop
 *              no split candidates:                 status HPSDF_CLEARANCE_DEPTH, stop
 *              otherwise the split candidates' eight children each, in list order, form list l + 1.
 *              A level's new finals follow the earlier ones in list order.
 *   At the end hi = best, lo = the minimum of blo over finals; finals with blo > hi are removed, their order kept, and counted in
 *   cells_pruned; out_cells holds what is left with cls = clsA, cells_open is their number.  With no witness hi = +inf and point, image
 *   and value_a are quiet NaNs.  Otherwise point = x of the witness, image = y, value_a = va and Query_B(image) == hi, bit for bit.
 *   cells_visited is the sum of the list lengths, levels the index of the last list.
 * Why it holds.  blo bounds Query_B at every y of the cell's image box that reaches B -- IntegratePair's argument with the same delta --
 * and the box holds the computed image of the cell's centre, so blo <= vb for a candidate.  hi is a value Query_B takes at the image of
 * a point of A's root with Query_A < iso_a: hi >= m.  A cell dropped by A's class holds no point with Query_A < iso_a (Integrate's
 * argument); a pruned cell has every value above a best that is >= m, or no value at all.  A point x with Query_A(x) < iso_a and a value
 * v = Query_B(M x + t) lies at every level in a cell with blo <= v < +inf; while v <= best that cell survives, so every point whose
 * value is at most the final hi -- the minimiser among them -- lies in a final cell, and lo <= m.  (The cell of the final witness is one
 * of them: blo <= vb = best.)  tol only stops the loop and is no part of the guarantee; the statuses CELL_LIMIT and DEPTH only leave a
 * wider enclosure.  lo is a statement about all x with Query_A(x) < iso_a: it is true even if that set is empty (then hi = +inf).
 * A non-finite pose entry, iso_a or tol, tol < 0, a range outside those above, a NULL tree, pose or `out`, only one of out_cells and
 * out_n_cells NULL, two trees on different devices: HPSDF_ERR_INVALID_ARGUMENT, and nothing is written.  tree_a == tree_b is allowed.
 * The cell array and its ownership are Integrate's.  hpsdf_clearance_device runs on the context stream -- per level a bound kernel (a
 * lane per cell, B walked with its stack in LDS, the (vb, pos) minimum reduced per workgroup in LDS, shuffles and DPP), a fold that
 * updates best in device memory, a prune kernel, a rocPRIM scan, one read-back and an emit kernel -- and synchronises before it returns;
 * no atomic decides a value.  _host computes on the calling thread from the trees' host copies, _block from two serialised blocks with
 * no device at all.
 * Batches.  hpsdf_clearance_batch_* answer n poses of the same two trees in one call: poses holds n x 12 doubles, out n structs, and
 * iso_a, depth, tol, max_cells and max_leaves are shared.  Every pose runs the rule above on its own -- pos is a cell's position in its
 * own pose's list -- and out[i] equals, byte for byte, what the single call returns for pose i; it does not depend on the other poses,
 * on their order or on max_total_cells.  One addition to the rule, the decision threshold `decide` (a quiet NaN: off; the single
 * entries run with it off): in step 3, after the test best - L <= tol and before the cell-limit test,
 *              L > decide or best < decide:         status HPSDF_CLEARANCE_DECIDED, the split candidates join finals, stop
 * L > decide proves that every point of A's solid has a B-value above decide, best < decide is a witness below it; the enclosure is
 * as guaranteed as any other, only wider than the full search's.  Arguments: those of the single call for every pose; decide finite or
 * a NaN; n <= 2^24 (n == 0 returns HPSDF_OK, writes nothing, and poses and out may be NULL); max_total_cells in max_cells .. 2^28, the
 * most cells the lists of all poses of one pass hold together.  The device entry takes the poses in chunks whose lists 0 fit that
 * budget (a single pose is always admitted); a chunk whose next list would not fit is halved and its parts start again from list 0.
 * On the device the lists of a chunk's poses are one list (a pose's cells contiguous, in the single call's order, with a parallel pose
 * index) and the levels run in lockstep: per level a bound kernel, a kernel that finds each pose's (vb, pos) minimum, a prune kernel,
 * a kernel that runs step 3's last lines a lane a pose, a kernel that writes the scan's words, one rocPRIM scan over the cells, an emit kernel and one read-back of two
 * totals -- a number of launches that does not depend on n.  The per-pose minima and counts are integer atomics (a minimum over an
 * order-preserving key of the double, then over pos; sums of counts): no result depends on the order of execution.  Batches do not
 * return cells.  hpsdf_clearance_batch_host and _block are a loop of the single call's host path with `decide`.
 * On HPSDF_ERR_INVALID_ARGUMENT nothing is written.
 * Not done: maximisation; cells from a batch (batches of poses return the structs only); subdiv above 1 on B; upper bounds
 * without a witness (an inside cell's walk gives a hi that no sample attains); best-first ordering of the cells; contact normals
 * (call QueryGradient of B at `image`). */
enum {
    HPSDF_CLEARANCE_CONVERGED = 0,
    HPSDF_CLEARANCE_DEPTH = 1,
    HPSDF_CLEARANCE_CELL_LIMIT = 2,
    HPSDF_CLEARANCE_EMPTY = 3,
    HPSDF_CLEARANCE_NOT_FINITE = 4,
    HPSDF_CLEARANCE_DECIDED = 5 /* the batch entries' `decide` only */
};
typedef struct hpsdf_clearance { /* 112 bytes */
    double lo, hi;            /* lo <= m <= hi */
    double point[3];          /* the witness in A's world frame */
    double image[3];          /* M point + t: Query_B there is hi */
    double value_a;           /* Query_A(point) < iso_a */
    uint64_t cells_visited;   /* the sum of the list lengths */
    uint64_t cells_outside_a; /* dropped by A's class */
    uint64_t cells_pruned;    /* dropped by their bound */
    uint64_t cells_open;      /* the final cells left: *out_n_cells */
    uint32_t status;          /* HPSDF_CLEARANCE_* */
    uint32_t levels;
} hpsdf_clearance;
HPSDF_API int hpsdf_clearance_device(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, const double pose[12], double iso_a,
                                     uint32_t depth, double tol, uint32_t max_cells, uint32_t max_leaves, hpsdf_clearance* out,
                                     hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_clearance_host(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, const double pose[12], double iso_a,
                                   uint32_t depth, double tol, uint32_t max_cells, uint32_t max_leaves, hpsdf_clearance* out,
                                   hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_clearance_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, const double pose[12], double iso_a,
                                    uint32_t depth, double tol, uint32_t max_cells, uint32_t max_leaves, hpsdf_clearance* out,
                                    hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells);
HPSDF_API int hpsdf_clearance_batch_device(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, const double* poses, size_t n,
                                           double iso_a, uint32_t depth, double tol, double decide, uint32_t max_cells, uint32_t max_leaves,
                                           uint32_t max_total_cells, hpsdf_clearance* out);
HPSDF_API int hpsdf_clearance_batch_host(hpsdf_ctx* ctx, const hpsdf_tree* tree_a, const hpsdf_tree* tree_b, const double* poses, size_t n,
                                         double iso_a, uint32_t depth, double tol, double decide, uint32_t max_cells, uint32_t max_leaves,
                                         uint32_t max_total_cells, hpsdf_clearance* out);
HPSDF_API int hpsdf_clearance_batch_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, const double* poses, size_t n,
                                          double iso_a, uint32_t depth, double tol, double decide, uint32_t max_cells, uint32_t max_leaves,
                                          uint32_t max_total_cells, hpsdf_clearance* out);

/* ---- Simplify: hp-coarsen a built tree within an RMS bound (no reference counterpart) ---------------------------------------------------
 * Makes a NEW tree from a serialised one: sibling leaves are merged into their parent (h-coarsening) and top degrees are dropped
 * (p-coarsening) wherever that keeps the result within `rms` of the source, cell by cell.  The source block is never written.  No field
 * sample is taken: everything is computed from the coefficients, and the error is bounded, not estimated.  The result is an ordinary
 * MemoryBlock -- hpsdf_tree_upload, the *_block entries and the reference's FromMemoryBlock / Query read it.
 * Why coefficients suffice.  In the root's normalised frame [-0.5, 0.5]^3 a cell at depth d has volume 8^-d, and a leaf's basis -- the
 * products of sqrt((2i+1) 2^d) P_i along each axis (NormalisedLengths, Utility.h:63-78) -- is orthonormal over its cell, and graded:
 * the rows of degree p are a prefix of the rows of degree p + 1.  So (1) dropping rows is the L2 projection and its squared L2 error is
 * the sum of the squares of the dropped rows; (2) the L2 projection of the polynomials of eight siblings onto one polynomial over their
 * parent is the separable map below, whose two 13 x 13 matrices do not depend on the depth; (3) the parent's polynomial restricted to
 * a child is the transposed map, so the projection's error is computable exactly as well.
 * Arguments: a block that hpsdf_query_bounds_block accepts; rms finite and >= 0; flags a combination of HPSDF_SIMPLIFY_MERGE and
 * HPSDF_SIMPLIFY_TRUNCATE (HPSDF_SIMPLIFY_DEFAULT = both).
 *   Tables     For the lower (s = 0) and the upper (s = 1) half of an axis and 0 <= j <= i <= 12
 *                T_s[i][j] = sqrt((2i+1)(2j+1)/2) * 1/2 * integral over [-1, 1] of P_i((t + 2s - 1) / 2) P_j(t) dt,
 *              0 above the diagonal; computed once on the host beyond long-double accuracy (a 16-point Gauss rule, nodes, recurrence and
 *              sum in double-double, the normalisation in long double) and rounded to double: hpsdf_simplify_transfer returns them.
 *              sum_s T_s T_s^T = I.  Bit a of a child's index selects the upper half on axis a (CornerAABB's convention).
 *   Entries    Entry (i, j, k) of a polynomial of degree q, i + j + k <= q, is its row in the basis's order.  A leaf of degree d stores
 *              count[d] rows; a row it does not store counts as 0 -- the rows above its degree, and (6, 0, 0) of a degree-6 leaf, whose
 *              count is 83 (the reference's table).
 *   e          Every leaf carries e, a bound on the squared L2 distance between the result and the SOURCE over its cell; 0 at first.
 *   Merge      (flag MERGE) For D = maxDepth .. 2, every interior node at depth D - 1 whose eight children are leaves -- leaves made
 *              at the level before included -- is a candidate.  q = the largest child degree.  For the entries (a, b, c) of degree q,
 *              over the children n = 0 .. 7 in that order, parent = parent + c_n's image, from 0.0:
 *                V[a, j, k] = sum_{i <= a} T_sx[a][i] c_n[i, j, k];  W[a, b, k] = sum_{j <= b} T_sy[b][j] V[a, j, k];
 *                image[a, b, c] = sum_{k <= c} T_sz[c][k] W[a, b, k]            (every sum from 0.0, its index ascending, s = T * x + s)
 *              An entry the degree q does not store is then set to 0.  The residual is the direct one: for n = 0 .. 7 the parent's
 *              restriction
 *                V[a, b, k] = sum_{c = k .. q-a-b} T_sz[c][k] parent[a, b, c];  W[a, j, k] = sum_{b = j .. q-a-k} T_sy[b][j] V[a, b, k];
 *                r_n[i, j, k] = sum_{a = i .. q-j-k} T_sx[a][i] W[a, j, k]
 *              and x[e] = x[e] + (c_n[e] - r_n[e])^2 per entry e, from 0.0; the x[e], zero-padded to the next power of two P, are summed
 *              by: for stride = P/2, P/4, .., 1: x[t] = x[t] + x[t + stride] for t < stride; e_step = x[0].  (Not sum |c_n|^2 - |parent|^2:
 *              the same number in exact arithmetic, but all cancellation once e_step is below 1e-16 of the energy.)
 *                b = (sqrt(e_step) + sqrt(((e_0 + e_1) + ..) + e_7))^2
 *              The merge is accepted iff b <= (rms * rms) * 8^-(D-1) and b is finite (a NaN fails the comparison): the node becomes a
 *              leaf of degree q with the parent's rows and e = b; its children are dropped.  The root stays interior: eight leaves
 *              at depth 1 (9 nodes) are the coarsest result.
 *   Truncate   (flag TRUNCATE) For every leaf of the result so far, of degree d at depth D: tail(d'') = the sum of the squares of its rows
 *              from count[d''] on, formed shell by shell from the top (a shell's squares in row order from 0.0; tail = tail + shell).
 *              For d'' = d - 1, d - 2, ..: b = (sqrt(tail(d'')) + sqrt(e))^2 with the leaf's e from the merge pass; while
 *              b <= (rms * rms) * 8^-D and b is finite the leaf's degree becomes d'' and its e becomes b; the first d'' that fails ends it.
 *   rms == 0   Both passes are skipped: the result is the source, re-serialised in the canonical order.
 *   Output     The surviving nodes keep their relative order (a node's new index is its rank among the survivors, so groups of eight
 *              siblings stay contiguous; nodes the source's root does not reach are not survivors), child_idx is remapped, a leaf's is
 *              all-ones; boxes and depths are the source's; the coefficients lie in the order of Octree::ReallocCoeffs
 *              (Octree.cpp:474-555), a depth-first walk with children 0 .. 7; the Config is copied unchanged.
 * Guarantee.  Every leaf cell C of the result satisfies  integral over C of (result - source)^2 <= e_C <= rms^2 vol(C), so the RMS
 * deviation over every leaf cell, and therefore over the root, is at most rms; the squared L2 deviation over the root is at most
 * error_bound = the sum of e_C.  Derivation, by induction over the steps: a leaf of the source has deviation 0 = e.  A merge replaces,
 * over the parent's cell, the current result g (within sqrt(sum e_n) of the source f in L2 over that cell, the children's cells being
 * disjoint) by the parent's polynomial h with |g - h|^2 = e_step computed directly; |f - h| <= |f - g| + |g - h| gives b.  A truncation
 * replaces a leaf's polynomial g by its prefix h with |g - h|^2 = tail exactly (orthonormal rows), and the same inequality applies.
 * Each accepted b satisfies the cell's threshold, so e_C <= rms^2 vol(C) at every step.  What is outside the statement: the float64
 * rounding of e_step, tail and the rows themselves (relative 1e-15 of the energy, not of the residual: a bound far below 1e-30 of a
 * cell's energy means "equal to rounding").
 * Limits, stated rather than hidden: the deviation measured is the UNWEIGHTED L2 norm -- a nearness-weighted Config is copied but
 * plays no part --, it is a mean-square bound per cell, not a pointwise one; a source that went through the continuity post-process
 * loses the enforced continuity wherever cells change.  Out of scope: a global error budget in place of the per-cell one; merging
 * into a degree above the children's; re-establishing continuity afterwards.
 * hpsdf_simplify runs on the context's device and stream (per level: simplify_candidates_kernel, one rocPRIM scan, simplify_list_kernel
 * and simplify_merge_kernel; simplify_truncate_kernel once at the end; csrc/simplify.hip) and synchronises before it returns; *out_block
 * comes from the context's block allocator, or malloc (the caller frees it), as for hpsdf_create.  hpsdf_simplify_block computes on the
 * calling thread with no device (csrc/simplify_host.cpp) and always mallocs.  Both run the statements of csrc/simplify.hpp in the order
 * written above (no multiply-add is fused) and return the same bytes and the same stats.  Blocks are accepted and refused as
 * hpsdf_query_bounds_block does.  rms negative or not finite, unknown flag bits, NULL out_block or out_size:
 * HPSDF_ERR_INVALID_ARGUMENT.  On any failure nothing is written and nothing stays allocated.  stats may be NULL. */
enum { HPSDF_SIMPLIFY_MERGE = 1, HPSDF_SIMPLIFY_TRUNCATE = 2 };
#define HPSDF_SIMPLIFY_DEFAULT (HPSDF_SIMPLIFY_MERGE | HPSDF_SIMPLIFY_TRUNCATE)
typedef struct hpsdf_simplify_stats {
    uint64_t nodes_in, coeffs_in, leaves_in;    /* the source, as its root reaches it */
    uint64_t nodes_out, coeffs_out, leaves_out; /* the result */
    uint64_t merges;      /* accepted merges, those whose leaf was merged again included */
    uint64_t truncations; /* leaves whose degree the truncation pass lowered */
    uint64_t levels;      /* levels of the merge pass that had a candidate */
    double error_bound;   /* the sum of e over the result's leaves: bounds the squared L2 deviation over the root */
    double max_cell_rms;  /* the largest sqrt(e / vol) over the result's leaves; <= rms */
} hpsdf_simplify_stats;
HPSDF_API int hpsdf_simplify(hpsdf_ctx* ctx, const void* block, size_t size, double rms, uint32_t flags, void** out_block, size_t* out_size,
                             hpsdf_simplify_stats* stats);
HPSDF_API int hpsdf_simplify_block(const void* block, size_t size, double rms, uint32_t flags, void** out_block, size_t* out_size,
                                   hpsdf_simplify_stats* stats);
HPSDF_API int hpsdf_simplify_transfer(double out[2][13][13]);

/* ---- Create: Octree::Create under the canonical round schedule ---------------
 * (Octree.cpp:312-352, 194-309, 558-659, 804-856, 1007-1093; schedule: DESIGN.md)
 *
 * One round = select jobs -> compute this rank's slice on the GPU -> (exchange
 * the 9 errors per job across ranks) -> apply.  The exchange is the caller's:
 * world == 1 needs none; N ranks all-gather the slice buffers over RCCL
 * (hp-adaptive-..._amd/distributed.py).  Every rank applies the same headers in
 * the same order, so all ranks hold identical trees. */
typedef struct hpsdf_build hpsdf_build;

typedef struct hpsdf_build_opts {
    uint64_t max_jobs_per_round; /* K of the canonical schedule; 0 = HPSDF_DEFAULT_JOBS_PER_ROUND */
    int32_t rank, world;         /* this process's shard of every round */
    int32_t reserved[2];
} hpsdf_build_opts;

typedef struct hpsdf_job { /* one popped heap entry (BuildThreadPool::Input, BuildThreadPool.h:24-28) */
    uint64_t node_idx;
    float aabb_min[3], aabb_max[3];
    double err;
    uint8_t degree, depth, coarse, pad[5];
} hpsdf_job;

#define HPSDF_JOB_HEADER_DOUBLES 9 /* p_err, h_err[0..7] */

typedef struct hpsdf_build_stats { /* 112 bytes since ABI 3, frozen (see HPSDF_ABI_VERSION) */
    uint64_t rounds, jobs, p_refines, h_refines, dropped, fits, samples;
    uint64_t n_nodes, n_leaves, n_coeffs;
    double total_error;  /* the reference's running float64 total (Octree.cpp:212, :257, :272, :276) as its stop rule reads it, not the sum
                            of the leaves' errors: round 0's 4096 additions to 409 600 leave a drift of 1e-9..1e-8 (bound 9e-8), so below
                            about 1e-8 it can end under the target, or negative, with the true sum far above it */
    uint64_t fit_mode;   /* HPSDF_FIT_* the build ran in */
    uint64_t split_fits; /* from-scratch fits whose rows below the top degree came from the sum-factorised / matrix-core kernel (HPSDF_FIT_SPLIT,
                            degree >= split_min_degree); 0: every coefficient is the bit-exact kernel's */
    uint64_t device_frontier; /* 1: selection, decision and bookkeeping ran on the device (csrc/frontier.hip, driven by csrc/frontier_build.cpp); 0: the host scheduler's rounds */
} hpsdf_build_stats;

HPSDF_API int hpsdf_build_begin(const hpsdf_config* cfg, const hpsdf_build_opts* opts, hpsdf_build** out);
HPSDF_API int hpsdf_build_destroy(hpsdf_build* b);
/* pops the next batch; *n_jobs == 0 means the stop rule fired (Octree.cpp:216) */
HPSDF_API int hpsdf_build_round_select(hpsdf_build* b, uint64_t* n_jobs);
HPSDF_API int hpsdf_build_round_jobs(const hpsdf_build* b, hpsdf_job* out);
/* contiguous cost-balanced job range of `rank`; identical on every rank */
HPSDF_API int hpsdf_build_round_slice(const hpsdf_build* b, int rank, uint64_t* first_job, uint64_t* n_jobs);
/* largest slice over ranks (padding unit of the all-gather) */
HPSDF_API int hpsdf_build_round_max_slice(const hpsdf_build* b, uint64_t* n_jobs);
/* sample + fit + error kernels for this rank's slice, asynchronous on the ctx stream */
HPSDF_API int hpsdf_build_round_compute(hpsdf_build* b, hpsdf_ctx* ctx, const hpsdf_field* field);
/* this rank's [slice][9] header buffer in HBM (valid until the next round_select) */
HPSDF_API int hpsdf_build_round_results_device(hpsdf_build* b, double** d_headers, uint64_t* n_doubles);
/* D2H of the same, synchronous */
HPSDF_API int hpsdf_build_round_results_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out);
/* headers of ALL jobs of the round, [n_jobs][9], host memory */
HPSDF_API int hpsdf_build_round_apply(hpsdf_build* b, const double* headers);
/* integration/test hook: supply one job's coefficients from the host instead of the GPU arena
 * (p_coeffs: ncoef(p+1) or 10 for a coarse job; h_coeffs: 8*ncoef(p); either may be NULL if unused) */
HPSDF_API int hpsdf_build_round_inject(hpsdf_build* b, uint64_t job, const double* p_coeffs,
                                       const double* h_coeffs);

/* Nearness-weighted builds on N ranks (config.weighting_type != 0, opts.world > 1).  A weighted fit keeps ONE full
 * coefficient array per node and an incremental fit copies the node's previous rows (Octree.cpp:847), so the rank
 * that fits a node next needs what another rank accepted for it: after every hpsdf_build_round_apply the ranks hand
 * each other the arrays that round accepted (a P refinement: the node's new array; an H refinement: its 8
 * children's), in job order.  hpsdf_build_rows_counts: doubles each rank contributes (all zero for unweighted or
 * single-rank builds); hpsdf_build_rows_pack_host: this rank's part, contiguous; after an all-gather,
 * hpsdf_build_rows_unpack_host(parts[world]) stores the other ranks' parts in this rank's arena (ctx != NULL) or host
 * store (ctx == NULL, CPU tests).  parts[own rank] is not read.  hpsdf_build_node_rows_host: the rows a node holds right
 * now, if this rank has them (out may be NULL to ask for the count). */
HPSDF_API int hpsdf_build_rows_counts(const hpsdf_build* b, uint64_t* counts_per_rank);
HPSDF_API int hpsdf_build_rows_pack_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out);
HPSDF_API int hpsdf_build_rows_unpack_host(hpsdf_build* b, hpsdf_ctx* ctx, const double* const* parts);
HPSDF_API int hpsdf_build_node_rows_host(hpsdf_build* b, hpsdf_ctx* ctx, uint64_t node_idx, double* out, uint64_t* n_rows);

/* ReallocCoeffs (Octree.cpp:474-555): DFS layout, then gather.  counts[r] = doubles owned by rank r. */
HPSDF_API int hpsdf_build_layout(hpsdf_build* b, uint64_t* n_coeffs_total, uint64_t* counts_per_rank);
/* this rank's leaves' coefficients, in DFS order */
HPSDF_API int hpsdf_build_pack_device(hpsdf_build* b, hpsdf_ctx* ctx, double** d_pack, uint64_t* n_doubles);
HPSDF_API int hpsdf_build_pack_host(hpsdf_build* b, hpsdf_ctx* ctx, double* out);
/* packs[r] = rank r's buffer (host).  *block is malloc'd; the caller frees it with free()
 * (ToMemoryBlock ownership, Octree.cpp:445; README.md:41). */
HPSDF_API int hpsdf_build_assemble(hpsdf_build* b, const double* const* packs, void** block, size_t* size);
HPSDF_API int hpsdf_build_get_stats(const hpsdf_build* b, hpsdf_build_stats* out);

/* ---- continuity post-process: Octree::PerformContinuityPostProcess (Octree.cpp:1717-1762) ------------
 * Host side, as the reference's (which hands the system to Eigen): enumerate the face-adjacent leaf pairs
 * (NodeProc/FaceProc, :1549-1612), assemble the jump-energy matrix M (analytic integrals for equal depths
 * :1459-1546, Gauss-Legendre ones otherwise :1250-1456), solve (M + strength I) x = strength c by
 * preconditioned CG from the guess strength c until |r| < tol |b| (the reference: tol = EPSILON_F32 with
 * Eigen's IncompleteCholesky; here Jacobi -- same solution to solver tolerance), overwrite the coefficients.
 * Deterministic for any thread count. */
typedef struct hpsdf_continuity_stats {
    uint64_t n_pairs, n_pairs_analytic, n_pairs_numeric, nnz, iterations;
    double residual;    /* |b - A x| / |b| at exit */
    double jump_before; /* c^T M c: jump energy of the fitted coefficients */
    double jump_after;  /* x^T M x */
    double assemble_ms, solve_ms;
} hpsdf_continuity_stats;
/* In place on a serialised block in host memory (the layout hpsdf_tree_upload takes); strength is read from
 * the block's Config.  tol <= 0: EPSILON_F32 (1e-6, Octree.cpp:1754); max_iter <= 0: 2n (Eigen's default);
 * threads 0: the block's config.thread_count (capped to the machine). */
HPSDF_API int hpsdf_continuity_post_process(void* block, size_t size, double tol, int max_iter, uint64_t threads,
                                            hpsdf_continuity_stats* stats);
/* The same on ctx's device (what hpsdf_create runs): assembly and conjugate-gradient loop in HBM, every entry and every
 * sum formed in the host path's order -- the block comes back bit-identical to hpsdf_continuity_post_process's.
 * (HPSDF_CONTINUITY_HOST_ASSEMBLY=1 in the environment keeps the assembly on the host.) */
HPSDF_API int hpsdf_continuity_post_process_device(hpsdf_ctx* ctx, void* block, size_t size, double tol, int max_iter,
                                                   uint64_t threads, hpsdf_continuity_stats* stats);
/* M itself (without the regularisation), CSR with duplicates summed; the three arrays are malloc'd, the
 * caller frees them.  Test / diagnostic hook. */
HPSDF_API int hpsdf_continuity_matrix(const void* block, size_t size, uint64_t threads, uint64_t** row_ptr,
                                      uint64_t** col, double** val, hpsdf_continuity_stats* stats);
/* The same matrix assembled on ctx's device (what hpsdf_create and hpsdf_continuity_post_process_device use) and copied
 * back: identical to hpsdf_continuity_matrix's arrays bit for bit.  HPSDF_ERR_UNSUPPORTED for trees the device assembly
 * leaves to the host (a leaf with more than 1024 face neighbours, own blocks beyond 2 GB). */
HPSDF_API int hpsdf_continuity_matrix_device(hpsdf_ctx* ctx, const void* block, size_t size, uint64_t** row_ptr, uint64_t** col,
                                             double** val, hpsdf_continuity_stats* stats);
/* stats of the last post-process hpsdf_create ran on this thread (zeros if it ran none) */
HPSDF_API int hpsdf_continuity_last_stats(hpsdf_continuity_stats* out);

/* Where the memory blocks of hpsdf_create / hpsdf_create_distributed come from.  By default they are malloc'd and the caller frees
 * them with free() -- MemoryBlock's contract (Utility.h: { size, ptr }, freed by the caller).  A host binding whose own block type
 * cannot adopt a malloc'd pointer (a Python bytes object, a Go slice, a JVM direct buffer) pays a second copy of the whole block for
 * that; with an allocator the library writes the block straight into the binding's memory: alloc(size, user) is called in place of
 * malloc(size) and the returned pointer comes back as *block (NULL: the build fails with HPSDF_ERR_OUT_OF_MEMORY).  A block the
 * build has begun but will not return (it allocates the block of a build that stops after the first round before it knows that the
 * build stops there; failures) goes to release(ptr, user).  Both are called on the thread that called Create, during the call.
 * alloc == NULL restores malloc / free.  (hpsdf_build_assemble always mallocs.) */
typedef void* (*hpsdf_block_alloc_fn)(size_t size, void* user);
typedef void (*hpsdf_block_release_fn)(void* block, void* user);
HPSDF_API void hpsdf_ctx_set_block_allocator(hpsdf_ctx* ctx, hpsdf_block_alloc_fn alloc, hpsdf_block_release_fn release, void* user);

/* whole Create on one GPU: begin .. assemble, then the continuity post-process when
 * cfg->continuity_enforce is set (Octree.cpp:341-344).  *block is malloc'd (caller frees) unless the context has a block allocator.
 * HPSDF_ERR_INVALID_ARGUMENT after the first round if the field is NaN or infinite at a sample point: the total error is then
 * NaN / infinite for good and the reference's loop (Octree.cpp:216) would refine until memory ends. */
HPSDF_API int hpsdf_create(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field,
                           uint64_t max_jobs_per_round, void** block, size_t* size, hpsdf_build_stats* stats);

/* ---- Create sharded over the GPUs of one node ---------------------------------------------------------------
 * One process (or thread) per GPU, each with its own context, all calling this with the same config, field and K.
 * Tree, frontier and field are replicated; every round's jobs are cut into `world` contiguous cost-balanced slices and
 * rank r fits slice r on its GPU; the ranks then exchange the 9 errors per job -- ONE all-gather per round -- and every
 * rank applies identical results in identical order; one more all-gather at the end reassembles the packed coefficient
 * store.  The block is byte-identical on every rank and identical to what world = 1 builds.
 * (Reference: there is no multi-process build; this is Octree::Create, Octree.cpp:312-352, with the job loop :194-309
 * sharded.)
 *
 * gather: in-place all-gather of equal parts on device memory -- rank r's contribution sits at
 * d_buf + r * bytes_per_rank when it is called; when the work it enqueues on `stream` (a hipStream_t) has run, every
 * rank's d_buf must hold all `world` parts.  It returns 0 on success.  With RCCL this is one call,
 *     ncclAllGather((char*)d_buf + rank * n, d_buf, n, ncclChar, comm, stream)      (include/hpsdf_rccl.hpp);
 * the library itself does not link RCCL.
 * Fields the device evaluates itself run the device-side frontier on up to 8 ranks (slices cut, errors decided and the tree
 * updated on every rank's GPU).  A nearness-weighted config does too (round 5): a weighted fit reads the cell's earlier rows, so
 * the round's part of the coefficient arena is laid out alike on every rank and exchanged as well -- one more call of `gather`
 * a round, in front of the errors' -- and nothing is exchanged at the end.  Host callbacks, logging, K > 4096 and worlds beyond 8
 * run the host scheduler's rounds, sharded the same way (same bytes): the exchanges are staged through a device buffer for the
 * same `gather`, and a weighted build hands the arrays each round accepted to every rank (hpsdf_build_rows_*).
 * The stepwise hpsdf_build_* calls expose the same loop to callers with a transport of their own.
 * stats: everything describes the whole build and is the same on every rank, except `fits` and `samples`, which count the rank's
 * own share (their sums over the ranks are the single-rank figures).
 * FAILURES: a rank whose share of a round fails on its own (device memory one GPU cannot serve) still enters the exchange the
 * other ranks are heading for, with a status word set in its part of the exchanged buffer, and then returns its error; every
 * other rank finds the status after the exchange and returns HPSDF_ERR_STATE naming the rank -- nobody is left waiting in a
 * collective (tests: test_a_failing_rank_takes_the_others_out_with_it).  What this cannot cover: a failure of the exchange
 * callback itself, a sticky device error (after which no further call succeeds), and the last exchange of the device-side
 * frontier (the packed coefficients, whose only local failure is the allocation of the packed store): there the caller must
 * abort the communicator when a rank reports an error, as for any collective program. */
typedef int (*hpsdf_allgather_fn)(void* user, void* d_buf, size_t bytes_per_rank, void* stream);
HPSDF_API int hpsdf_create_distributed(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field,
                                       uint64_t max_jobs_per_round, int rank, int world, hpsdf_allgather_fn gather,
                                       void* user, void** block, size_t* size, hpsdf_build_stats* stats);

/* ---- steady-state micro-benchmark hook (bench.py / profiles) ------------------
 * n_cells from-scratch fits of `degree` at `depth` over a lattice of cells, results discarded. */
HPSDF_API int hpsdf_bench_fit(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree,
                              int depth, uint64_t n_cells, int repeats, double* ms_per_launch);
/* The same fits with their results: Octree::FitPolynomial (Octree.cpp:1007-1093) from scratch at `degree` for the first
 * n_cells cells of the depth-`depth` lattice over [-1/2, 1/2]^3 (x fastest): coeffs[n_cells][ncoef(degree)], errs[n_cells].
 * The kernels are the ones a build would take in the context's fit mode (hpsdf_ctx_set_fit_mode).
 * What the fit known-answer tests compare with the oracle's FitPolynomial, degree by degree. */
HPSDF_API int hpsdf_fit_cells(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree, int depth,
                              uint64_t n_cells, double* coeffs, double* errs);

#ifdef __cplusplus
}
#endif
#endif /* HPSDF_H */
