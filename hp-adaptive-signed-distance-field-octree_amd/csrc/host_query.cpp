// Scalar-sized Query / QueryWithGradient calls, answered where the caller is.
//
// The reference's Octree::Query(pt) (Source/HP/Octree.cpp:662-702) costs ~75 ns and its own tests and benchmarks call it in loops
// of 1 M - 8 M points (Source/Tests/HPUnitTests.cpp:64-75, Source/Benchmarks/HPBenchmarks.cpp:105-109).  Through a kernel launch
// a one-point call is ~15 us whatever the kernel does, so calls of up to kHostQueryPoints points are evaluated here, on the
// calling thread, from the copy of the block's node array and coefficients the tree handle keeps (hpsdf_tree_upload) -- the
// same statements in the same order as queryPoint (leaf_eval.hpp) / queryPointWithGradient (kernels.hip) (and this file is compiled with
// -ffp-contract=off like everything else), so the values are the kernels' bit for bit (tests/test_gpu_parity.py compares them
// on the edge-point set).  It is not a CPU build of the library: a tree handle only exists on a device context, Create, the
// fields and every batched call are GPU code, and there is no entry point that works without a GPU.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "block.hpp"
#include "dual_vertex.hpp"
#include "edge_vertex.hpp"
#include "integrate.hpp"
#include "lattice_check.hpp"
#include "leaf_jet.hpp"
#include "ray_cast.hpp"
#include "runtime.hpp"
#include "tables.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

struct Leaf {
    const double* co;
    int degree, depth;
    double u[3];  // (pt - centre) * (2 << depth), Octree.cpp:862
};

// Octree.cpp:675-701, the mid-plane descent from a point p of the unit cube (>= takes the upper child): the record of the leaf it ends
// in, that leaf's centre in c, a quarter of its edge in q and its depth.  (interior: a = first child; leaf: a = offset in the line-aligned
// coefficient mirror, b = degree)
inline const NodeRec& walk(const hpsdf_tree& t, const double* p, double (&c)[3], double& q, int& depth) {
    c[0] = c[1] = c[2] = 0.0, q = 0.25, depth = 0;  // cell centres are exact dyadics: the mid-planes of the f32 boxes
    const NodeRec* nodes = t.hRecs.data();
    uint64_t idx = 0;
    while (nodes[idx].b == kInteriorTag) {
        uint64_t next = nodes[idx].a;
        for (int a = 0; a < 3; ++a) {
            const bool up = p[a] >= c[a];
            next += up ? (1ull << a) : 0ull;
            c[a] = up ? c[a] + q : c[a] - q;
        }
        q = q * 0.5;
        ++depth;
        idx = next;
    }
    return nodes[idx];
}

// Octree.cpp:665-701: root remap, f32 containment (both ends inclusive, NaN fails), then the walk
inline bool descend(const hpsdf_tree& t, const double* xyz, Leaf& L) {
    const double p[3] = {(xyz[0] - t.dev.rootCentre[0]) * t.dev.rootInvSizes[0], (xyz[1] - t.dev.rootCentre[1]) * t.dev.rootInvSizes[1],
                         (xyz[2] - t.dev.rootCentre[2]) * t.dev.rootInvSizes[2]};
    const float fx = (float)p[0], fy = (float)p[1], fz = (float)p[2];
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) return false;
    double c[3], q;
    int depth;
    const NodeRec& leaf = walk(t, p, c, q, depth);
    const double s = (double)(2 << depth);
    L.co = t.hPadded.data() + leaf.a;
    L.degree = (int)leaf.b;
    L.depth = depth;
    for (int a = 0; a < 3; ++a) L.u[a] = (p[a] - c[a]) * s;
    return true;
}

// the leaf's polynomial with its derivatives up to ORDER (leaf_jet.hpp), from the process's tables
template <int ORDER>
inline double leafValue(const Leaf& L, GradOut<ORDER> gu, HessOut<ORDER> hu) {
    const Tables& T = tables();
    return leafJet<ORDER>(
        L.co, AnyDegree{L.degree}, (int)T.coeffCount[L.degree], L.u, L.depth, &T.normalisedLengths[0][0], &T.recurrence[0][0],
        [&T](int r, int k) { return (int)T.basisIndex[r][k]; }, gu, hu);
}

}  // namespace

// Octree::Query + FApprox (Octree.cpp:662-702, 859-901)
double hostQueryPoint(const hpsdf_tree& t, const double* xyz) {
    Leaf L;
    if (!descend(t, xyz, L)) return DBL_MAX;
    return leafValue<0>(L, NoOutput{}, NoOutput{});
}

// Octree::QueryWithGradient + FApproxWithGradient (Octree.cpp:749-789, 904-985).  Outside the root: *out = DBL_MAX, grad untouched.
void hostQueryPointWithGradient(const hpsdf_tree& t, const double* xyz, double* out, double* grad, int leftAssoc) {
    Leaf L;
    if (!descend(t, xyz, L)) {
        *out = DBL_MAX;
        return;
    }
    const Tables& T = tables();
    const double eps = 0.0001;
    double Lg[13][3][3];
    for (int a = 0; a < 3; ++a) {
        const double u = L.u[a];  // :907
        Lg[0][a][0] = Lg[0][a][1] = Lg[0][a][2] = T.normalisedLengths[0][L.depth];
        double a2 = 0.0, a1 = 1.0, b2 = 0.0, b1 = 1.0, c2 = 0.0, c1 = 1.0;
        for (int j = 1; j <= L.degree; ++j) {
            const double r0 = T.recurrence[j][0], r1 = T.recurrence[j][1], nl = T.normalisedLengths[j][L.depth];
            const double a0 = r0 * u * a1 - r1 * a2;          // :937
            const double b0 = r0 * (u + eps) * b1 - r1 * b2;  // :941
            const double c0 = r0 * (u - eps) * c1 - r1 * c2;  // :945
            a2 = a1, a1 = a0, b2 = b1, b1 = b0, c2 = c1, c1 = c0;
            Lg[j][a][0] = a0 * nl, Lg[j][a][1] = b0 * nl, Lg[j][a][2] = c0 * nl;
        }
    }
    const int nc = (int)T.coeffCount[L.degree];
    double g[3];
    for (int k = 0; k < 3; ++k) {  // :956-968
        double p1 = 0.0, m1 = 0.0;
        for (int r = 0; r < nc; ++r) {
            p1 = p1 + L.co[r] * Lg[T.basisIndex[r][k]][k][1];
            m1 = m1 + L.co[r] * Lg[T.basisIndex[r][k]][k][2];
        }
        g[k] = (p1 - m1) / (2.0 * eps);
    }
    unitGradient(g, leftAssoc);  // Eigen normalize()
    double f = 0.0;  // :972-984
    for (int r = 0; r < nc; ++r) {
        double lp = Lg[T.basisIndex[r][0]][0][0];
        lp = lp * Lg[T.basisIndex[r][1]][1][0];
        lp = lp * Lg[T.basisIndex[r][2]][2][0];
        f = f + L.co[r] * lp;
    }
    *out = f;
    grad[0] = g[0], grad[1] = g[1], grad[2] = g[2];
}

// Octree::QueryRay (Octree.cpp:705-746; Ray::IntersectAABB, Source/Utility/Ray.cpp:18-68): the statements of query_ray_kernel
// (kernels.hip) -- the origin moved to the unit cube, the direction left as it is, the first intersection with [-0.5, 0.5]^3 unless the
// origin lies inside, then at most 200 steps of Query at the stepped point (Query maps to the unit cube AGAIN, as the reference's
// call does).  *tOut is written on a hit only.
bool hostQueryRay(const hpsdf_tree& t, const double* origin, const double* dir, double tMax, double* tOut) {
    double o[3], d[3], inv[3];
    int sgn[3];
    for (int a = 0; a < 3; ++a) {
        o[a] = (origin[a] - t.dev.rootCentre[a]) * t.dev.rootInvSizes[a];  // :711
        d[a] = dir[a];
        inv[a] = 1.0 / d[a];  // Ray.cpp:10 cwiseInverse
        sgn[a] = inv[a] < 0.0 ? 1 : 0;
    }
    double im[3] = {o[0], o[1], o[2]};  // intMin
    const float fx = (float)o[0], fy = (float)o[1], fz = (float)o[2];
    const bool inside = fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f;
    if (!inside) {
        double a0 = ((sgn[0] ? 0.5 : -0.5) - o[0]) * inv[0], b0 = ((sgn[0] ? -0.5 : 0.5) - o[0]) * inv[0];
        const double a1 = ((sgn[1] ? 0.5 : -0.5) - o[1]) * inv[1], b1 = ((sgn[1] ? -0.5 : 0.5) - o[1]) * inv[1];
        if ((a0 > b1) || (a1 > b0)) return false;
        if (a1 > a0) a0 = a1;
        if (b1 < b0) b0 = b1;
        const double a2 = ((sgn[2] ? 0.5 : -0.5) - o[2]) * inv[2], b2 = ((sgn[2] ? -0.5 : 0.5) - o[2]) * inv[2];
        if ((a0 > b2) || (a2 > b0)) return false;
        if (a2 > a0) a0 = a2;
        im[0] = a0, im[1] = a1, im[2] = a2;
    }
    const double eps = 0.0001, minStep = 0.0001;
    double dist = 0.0;
    for (int s = 0; s < 200; ++s) {
        const double p[3] = {im[0] + dist * d[0], im[1] + dist * d[1], im[2] + dist * d[2]};
        const double v = hostQueryPoint(t, p);
        if (v < eps) {
            *tOut = v;  // :730
            return true;
        }
        dist = dist + (v * 0.95 + minStep);  // :736
        if (dist > tMax) break;
    }
    return false;
}

namespace {

// QueryGradient (include/hpsdf.h): Query's descent, then the value and the gradient of the leaf's polynomial with the statements the
// kernels run (leaf_jet.hpp; query_gradient.hip).  Outside the root: DBL_MAX and three quiet NaNs.
void hostQueryPointTrueGradient(const hpsdf_tree& t, const double* xyz, bool unit, int leftAssoc, double* out, double* grad) {
    Leaf L;
    if (!descend(t, xyz, L)) {
        if (out) *out = DBL_MAX;
        grad[0] = grad[1] = grad[2] = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    double gu[3], g[3];
    const double f = leafValue<1>(L, gu, NoOutput{});
    finishTrueGradient(gu, L.depth, t.dev.rootInvSizes, unit, leftAssoc, g);
    if (out) *out = f;
    grad[0] = g[0], grad[1] = g[1], grad[2] = g[2];
}

// QueryHessian (include/hpsdf.h): Query's descent, then value, gradient, second derivative and curvature with the statements the kernels
// run (leaf_jet.hpp; query_hessian.hip).  Every output may be null.  Outside the root: DBL_MAX and quiet NaNs.
[[gnu::noinline]] void hostQueryPointHessian(const hpsdf_tree& t, const double* xyz, bool unit, int leftAssoc, double* out, double* grad,
                                             double* hess, double* curv) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double f = DBL_MAX, g[3] = {nan, nan, nan}, H[6] = {nan, nan, nan, nan, nan, nan}, k[2] = {nan, nan};
    Leaf L;
    if (descend(t, xyz, L)) {
        double gu[3], hu[6];
        f = leafValue<2>(L, gu, hu);
        finishTrueGradient(gu, L.depth, t.dev.rootInvSizes, false, leftAssoc, g);
        finishHessian(hu, L.depth, t.dev.rootInvSizes, H);
        if (curv) levelSetCurvature(g, H, leftAssoc, k);
        if (unit) unitGradient(g, leftAssoc);
    }
    if (out) *out = f;
    if (grad) grad[0] = g[0], grad[1] = g[1], grad[2] = g[2];
    if (hess)
        for (int a = 0; a < 6; ++a) hess[a] = H[a];
    if (curv) curv[0] = k[0], curv[1] = k[1];
}

// row i of an optional output array with `stride` elements a row (null stays null)
template <typename T>
inline T* rowOf(T* p, size_t i, size_t stride = 1) {
    return p ? p + stride * i : nullptr;
}

}  // namespace

// The rows of a call answered on the calling thread: what the *_host entries (capi_tree.cpp, up to kHostQueryPoints / kHostRays rows) and the
// *_block entries below run.  The optional outputs are passed as they came in.  The per-row routines with a single caller are kept out of line
// ([[gnu::noinline]]): compiled into its row loop hostCastRay spilt more of its walk's state, and a one-ray call is what the C++ drop-in's
// scalar CastRay costs (the instruction counts and the timings: profiles/point_call_plumbing_timing.txt, part B).
void hostTrueGradientRows(const hpsdf_tree& t, const double* xyz, size_t n, uint32_t flags, int leftAssoc, double* out, double* grad) {
    for (size_t i = 0; i < n; ++i)
        hostQueryPointTrueGradient(t, xyz + 3 * i, (flags & HPSDF_GRADIENT_UNIT) != 0u, leftAssoc, rowOf(out, i), grad + 3 * i);
}

void hostHessianRows(const hpsdf_tree& t, const double* xyz, size_t n, uint32_t flags, int leftAssoc, double* out, double* grad, double* hess,
                     double* curv) {
    for (size_t i = 0; i < n; ++i)
        hostQueryPointHessian(t, xyz + 3 * i, (flags & HPSDF_GRADIENT_UNIT) != 0u, leftAssoc, rowOf(out, i), rowOf(grad, i, 3), rowOf(hess, i, 6),
                              rowOf(curv, i, 2));
}

// what hpsdf_query_hessian_* reject before anything runs (0: fine)
int hessianArgumentError(uint32_t flags, const double* xyz, size_t n, const double* hess, const double* curv) {
    if (flags & ~HPSDF_GRADIENT_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_hessian: unknown flag bits");
    if (n && !xyz) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (!hess && !curv) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_hessian: hess and curv are both null");
    return HPSDF_OK;
}

namespace {

// ProjectToSurface (include/hpsdf.h) for one point: the loop of project.hip's projectPoint on hostQueryPointTrueGradient.  xyz and outXyz
// may be the same three doubles; every output but outXyz may be null.
[[gnu::noinline]] void hostProjectPoint(const hpsdf_tree& t, const double* xyz, double iso, double tol, uint32_t maxIter, bool unit, int leftAssoc,
                                        double* outXyz, double* outVal, double* outGrad, uint8_t* outIters, uint8_t* outStatus) {
    double x[3] = {xyz[0], xyz[1], xyz[2]}, f, g[3];
    uint32_t k = 0;
    int status;
    for (;;) {
        hostQueryPointTrueGradient(t, x, false, leftAssoc, &f, g);
        status = projectStep(f, g, iso, tol, k, maxIter, leftAssoc, x);
        if (status >= 0) break;
        ++k;
    }
    if (unit) unitGradient(g, leftAssoc);
    outXyz[0] = x[0], outXyz[1] = x[1], outXyz[2] = x[2];
    if (outVal) *outVal = f;
    if (outGrad) outGrad[0] = g[0], outGrad[1] = g[1], outGrad[2] = g[2];
    if (outIters) *outIters = (uint8_t)k;
    if (outStatus) *outStatus = (uint8_t)status;
}

}  // namespace

void hostProjectRows(const hpsdf_tree& t, const double* xyz, size_t n, double iso, double tol, uint32_t maxIter, uint32_t flags, int leftAssoc,
                     double* outXyz, double* outVal, double* outGrad, uint8_t* outIters, uint8_t* outStatus) {
    for (size_t i = 0; i < n; ++i)
        hostProjectPoint(t, xyz + 3 * i, iso, tol, maxIter, (flags & HPSDF_PROJECT_UNIT) != 0u, leftAssoc, outXyz + 3 * i, rowOf(outVal, i),
                         rowOf(outGrad, i, 3), rowOf(outIters, i), rowOf(outStatus, i));
}

// what hpsdf_project_* reject before anything runs (0: fine)
int projectArgumentError(uint32_t flags, double iso, double tol, uint32_t maxIter) {
    if (flags & ~HPSDF_PROJECT_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_project: unknown flag bits");
    if (!(tol >= 0.0)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_project: tol must be >= 0");
    if (!std::isfinite(iso)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_project: iso must be finite");
    if (maxIter > 255u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_project: max_iter must be <= 255");
    return HPSDF_OK;
}

namespace {

// what castRay (ray_cast.hpp) needs of a tree on the calling thread: QueryGradient at a world point, and the box of the leaf that
// Query's descent reaches from a point of the unit cube (descend's walk; the boxes are the exact dyadics it recomputes)
struct HostCastField {
    const hpsdf_tree& t;
    int leftAssoc;
    double eval(const double (&x)[3], double (&g)[3]) const {
        double f;
        hostQueryPointTrueGradient(t, x, false, leftAssoc, &f, g);
        return f;
    }
    void locate(const double (&pu)[3], double (&lo)[3], double (&hi)[3], int& degree) const {
        double c[3], q;
        int depth;  // (not needed here; walk is inlined and the count goes with it)
        degree = (int)walk(t, pu, c, q, depth).b;
        const double h = q + q;
        for (int a = 0; a < 3; ++a) lo[a] = c[a] - h, hi[a] = c[a] + h;
    }
};

inline uint16_t saturate16(uint32_t v) { return (uint16_t)(v > 65535u ? 65535u : v); }

// CastRays (include/hpsdf.h) for one ray: castRay (ray_cast.hpp) over the routines above.  Every output but outStatus may be null.
[[gnu::noinline]] void hostCastRay(const hpsdf_tree& t, const double* origin, const double* dir, double tMax, const CastArgs& a, int leftAssoc,
                                   uint8_t* outStatus, double* outT, double* outXyz, double* outVal, double* outGrad, uint16_t* outEvals,
                                   uint16_t* outCells) {
    HostCastField F{t, leftAssoc};
    CastRow r;
    castRay(F, t.dev.rootCentre, t.dev.rootInvSizes, leftAssoc, origin, dir, tMax, a, r);
    *outStatus = (uint8_t)r.status;
    if (outT) *outT = r.t;
    if (outXyz) outXyz[0] = r.x[0], outXyz[1] = r.x[1], outXyz[2] = r.x[2];
    if (outVal) *outVal = r.f;
    if (outGrad) outGrad[0] = r.g[0], outGrad[1] = r.g[1], outGrad[2] = r.g[2];
    if (outEvals) *outEvals = saturate16(r.evals);
    if (outCells) *outCells = saturate16(r.cells);
}

}  // namespace

void hostCastRows(const hpsdf_tree& t, const double* origins, const double* dirs, const double* tMax, size_t n, const CastArgs& a, int leftAssoc,
                  uint8_t* outStatus, double* outT, double* outXyz, double* outVal, double* outGrad, uint16_t* outEvals, uint16_t* outCells) {
    for (size_t i = 0; i < n; ++i)
        hostCastRay(t, origins + 3 * i, dirs + 3 * i, tMax[i], a, leftAssoc, outStatus + i, rowOf(outT, i), rowOf(outXyz, i, 3), rowOf(outVal, i),
                    rowOf(outGrad, i, 3), rowOf(outEvals, i), rowOf(outCells, i));
}

// what hpsdf_cast_rays_* reject before anything runs (0: fine)
int castArgumentError(uint32_t flags, double iso, double tol, uint32_t maxIter, uint32_t maxCells, size_t n, const void* origins, const void* dirs,
                      const void* tMax, const void* outStatus) {
    if (flags & ~HPSDF_CAST_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_cast_rays: unknown flag bits");
    if (!(tol >= 0.0)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_cast_rays: tol must be >= 0");
    if (!std::isfinite(iso)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_cast_rays: iso must be finite");
    if (maxIter > 255u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_cast_rays: max_iter must be <= 255");
    if (maxCells < 1u || maxCells > 65535u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_cast_rays: max_cells must be in 1..65535");
    if (n && (!origins || !dirs || !tMax || !outStatus)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return HPSDF_OK;
}

// QueryBounds (include/hpsdf.h) for n boxes: boundsWalk (tree_bound.hpp) with Query's leaf evaluation, the statements of
// query_bounds_kernel.  boxes == nullptr: the cells of *grid.  outLeaves may be null.
namespace {

template <class Boxes>
void boundsRows(const ClsTree& t, const Boxes& boxes, size_t n, uint32_t subdiv, uint32_t maxLeaves, double* outLo, double* outHi,
                uint8_t* outStatus, uint32_t* outLeaves) {
    const HostEval eval{&tables()};
    HostBoundsStack st;
    for (size_t i = 0; i < n; ++i) {
        double a[3], b[3];
        boxes.get(i, a, b);
        BoundsRow r;
        boundsWalk(t, a, b, subdiv, maxLeaves, eval, st, r);
        outLo[i] = r.lo, outHi[i] = r.hi, outStatus[i] = (uint8_t)r.status;
        if (outLeaves) outLeaves[i] = r.leaves;
    }
}

}  // namespace

void hostBoundsRows(const ClsTree& t, const double* boxes, const BoxGrid* grid, size_t n, uint32_t subdiv, uint32_t maxLeaves, double* outLo,
                    double* outHi, uint8_t* outStatus, uint32_t* outLeaves) {
    if (n == 0) return;  // (then both sources may be null)
    if (boxes)
        boundsRows(t, BoxArray{boxes}, n, subdiv, maxLeaves, outLo, outHi, outStatus, outLeaves);
    else
        boundsRows(t, *grid, n, subdiv, maxLeaves, outLo, outHi, outStatus, outLeaves);
}

// what hpsdf_query_bounds_* reject before anything runs (0: fine)
int boundsArgumentError(uint32_t subdiv, uint32_t maxLeaves, size_t n, const void* in, const void* lo, const void* hi, const void* status) {
    if (subdiv != 1u && subdiv != 2u && subdiv != 4u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_bounds: subdiv must be 1, 2 or 4");
    if (maxLeaves < 1u || maxLeaves > 65535u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_bounds: max_leaves must be in 1..65535");
    if (n && (!in || !lo || !hi || !status)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return HPSDF_OK;
}

// Integrate (include/hpsdf.h) on the calling thread: integrateLevels over host lists (integrate.hpp, HostIntegrateLists), with Query's leaf
// evaluation -- the statements of the kernels of integrate.hip, the rows reduced by the same rule.
namespace {

struct HostIntegrateCells {
    const ClsTree& t;
    const IntegrateArgs& a;
    HostEval eval;
    uint32_t cls(const IntegrateCell& c, int level, bool* finite) { return integrateCellClass(t, c, level, a.iso, eval, finite); }
    void row(const IntegrateCell& c, int level, double (&row)[kIntRow]) { integrateCellRow(t, c, level, a.iso, a.samples, eval, row); }
};

}  // namespace

int hostIntegrate(const ClsTree& t, size_t nNodes, const IntegrateArgs& a, hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HostIntegrateCells cells{t, a, HostEval{&tables()}};
    return hostIntegrateLists(cells, t, nNodes, a, out, outCells, outCount);
}

// what hpsdf_integrate_* reject before anything runs (0: fine)
int integrateArgumentError(double iso, uint32_t depth, uint32_t samples, uint32_t maxCells, const void* out, const void* outCells, const void* outCount) {
    if (!(std::fabs(iso) <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate: iso must be finite");
    if (depth > 15u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate: depth must be in 0..15");
    if (samples != 1u && samples != 2u && samples != 4u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate: samples must be 1, 2 or 4");
    if (maxCells < 8u || maxCells > (1u << 28)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate: max_cells must be in 8..2^28");
    if (!out || (outCells != nullptr) != (outCount != nullptr)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return HPSDF_OK;
}

namespace {

// What the *_block entries answer from: a serialised block as a host-only tree handle -- validated and laid out like the device mirror
// (block.hpp), so the descent and the evaluation are the code above -- and, there being no context, the process-wide reduction order.
int treeFromBlock(const void* block, size_t size, hpsdf_tree& t, int& leftAssoc) {
    BlockView v;
    BlockMirror m;
    std::string why;
    int rc = readBlock(block, size, v, why);
    if (!rc) rc = mirrorBlock(v, tables(), m, why);
    if (rc) return fail(rc, why);
    t.hRecs = std::move(m.recs);
    t.hPadded = std::move(m.padded);
    for (int a = 0; a < 3; ++a) t.dev.rootCentre[a] = m.rootCentre[a], t.dev.rootInvSizes[a] = m.rootInvSizes[a];
    leftAssoc = reductionLeftAssoc(nullptr);
    return HPSDF_OK;
}

// ExtractSurfaceDual (include/hpsdf.h) on the calling thread: the phases of surface_dual.hip as loops -- the lattice values through
// hostQueryPoint, the three bit words and their prefixes, a record a crossing edge through edgeVertex and hostQueryPointTrueGradient,
// a vertex a mixed cube through dual_vertex.hpp, two triangles an interior crossing edge.  The outputs are malloc'd last: nothing is
// allocated on an error.
struct BitWords {
    std::vector<uint64_t> words, prefix;  // prefix[w]: set bits in the words before w; prefix.back(): all of them
    explicit BitWords(uint64_t bits) : words((bits + 63) / 64, 0), prefix((bits + 63) / 64 + 1, 0) {}
    void set(uint64_t i) { words[i >> 6] |= 1ull << (i & 63u); }
    bool test(uint64_t i) const { return (words[i >> 6] >> (i & 63u)) & 1u; }
    void scan() {
        for (size_t w = 0; w < words.size(); ++w) prefix[w + 1] = prefix[w] + (uint64_t)__builtin_popcountll(words[w]);
    }
    uint64_t rank(uint64_t i) const { return prefix[i >> 6] + (uint64_t)__builtin_popcountll(words[i >> 6] & ((1ull << (i & 63u)) - 1ull)); }
    uint64_t count() const { return prefix.back(); }
};

int hostExtractSurfaceDual(const hpsdf_tree& t, const CheckedLattice& cl, double iso, double tau, int leftAssoc, double** verts, uint64_t* nVerts,
                           uint64_t** tris, uint64_t* nTris, uint8_t** vertInfo, double* values) {
    const uint32_t n[3] = {cl.n[0], cl.n[1], cl.n[2]}, np[3] = {cl.n[0] + 1u, cl.n[1] + 1u, cl.n[2] + 1u};
    const uint32_t stride[3] = {1u, np[0], np[0] * np[1]};
    const uint64_t nPts = cl.nPts, nEdges = 3 * nPts, nCubes = cl.nCubes;
    std::vector<double> v(nPts);
    for (uint64_t L = 0; L < nPts; ++L) {
        const uint32_t i = (uint32_t)(L % np[0]), r = (uint32_t)(L / np[0]), j = r % np[1], k = r / np[1];
        const double x[3] = {cl.lo[0] + (double)i * cl.h[0], cl.lo[1] + (double)j * cl.h[1], cl.lo[2] + (double)k * cl.h[2]};
        v[L] = hostQueryPoint(t, x);
    }
    const auto edgeOf = [&](uint64_t e, uint32_t& L, uint32_t& a, uint32_t (&idx)[3]) {
        L = (uint32_t)(e / 3u), a = (uint32_t)(e - 3u * (uint64_t)L);
        idx[0] = L % np[0], idx[1] = (L / np[0]) % np[1], idx[2] = (L / np[0]) / np[1];
    };
    BitWords crossing(nEdges), interior(nEdges), mixed(nCubes);
    for (uint64_t e = 0; e < nEdges; ++e) {
        uint32_t L, a, idx[3];
        edgeOf(e, L, a, idx);
        if (idx[a] >= n[a] || (v[L] < iso) == (v[L + stride[a]] < iso)) continue;
        crossing.set(e);
        if (dualInterior(idx, a, n)) interior.set(e);
    }
    const uint32_t cornerOff[8] = {0u, 1u, stride[1], stride[1] + 1u, stride[2], stride[2] + 1u, stride[2] + stride[1], stride[2] + stride[1] + 1u};
    const auto cubeBase = [&](uint64_t Q, uint32_t (&idx)[3]) {
        idx[0] = (uint32_t)(Q % n[0]), idx[1] = (uint32_t)((Q / n[0]) % n[1]), idx[2] = (uint32_t)((Q / n[0]) / n[1]);
        return idx[0] + np[0] * (idx[1] + np[1] * idx[2]);
    };
    for (uint64_t Q = 0; Q < nCubes; ++Q) {
        uint32_t idx[3], c = 0;
        const uint32_t L0 = cubeBase(Q, idx);
        for (int b = 0; b < 8; ++b) c |= (v[L0 + cornerOff[b]] < iso ? 1u : 0u) << b;
        if (c != 0u && c != 255u) mixed.set(Q);
    }
    crossing.scan(), interior.scan(), mixed.scan();
    const uint64_t E = crossing.count(), V = mixed.count(), T = 2 * interior.count();

    std::vector<DualRecord> recs(E);
    for (uint64_t e = 0; e < nEdges; ++e) {
        if (!crossing.test(e)) continue;
        uint32_t L, a, idx[3];
        edgeOf(e, L, a, idx);
        DualRecord& r = recs[crossing.rank(e)];
        edgeVertex(cl.lo, cl.h, idx, a, v[L], v[L + stride[a]], iso, r.p);
        hostQueryPointTrueGradient(t, r.p, false, leftAssoc, &r.f, r.g);
        r.pad = 0.0;
    }
    struct Malloced {  // released unless handed to the caller
        void* p = nullptr;
        ~Malloced() { std::free(p); }
    } hVerts, hTris, hInfo;
    if (V > 0) {
        hVerts.p = std::malloc(V * 3 * sizeof(double));
        if (T > 0) hTris.p = std::malloc(T * 3 * sizeof(uint64_t));
        if (vertInfo) hInfo.p = std::malloc(V);
        if (!hVerts.p || (T > 0 && !hTris.p) || (vertInfo && !hInfo.p))
            return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_extract_surface_dual_block: host allocation failed");
    }
    double* outV = (double*)hVerts.p;
    uint64_t* outT = (uint64_t*)hTris.p;
    uint8_t* outI = (uint8_t*)hInfo.p;
    for (uint64_t Q = 0, vtx = 0; Q < nCubes; ++Q) {
        if (!mixed.test(Q)) continue;
        uint32_t idx[3], k = 0;
        const uint32_t L0 = cubeBase(Q, idx);
        const DualRecord* rec[12];
        DualNormal N;
        double sum[3], m[3];
        dualClear(N, sum);
        for (uint32_t e = 0; e < 12u; ++e) {
            const uint64_t ge = 3u * (uint64_t)(L0 + cornerOff[dualEdgeCorner(e)]) + dualEdgeAxis(e);
            if (!crossing.test(ge)) continue;
            rec[k] = &recs[crossing.rank(ge)];
            dualAddPoint(rec[k]->p, sum);
            ++k;
        }
        dualMean(sum, k, m);
        for (uint32_t c = 0; c < k; ++c) dualAccumulate(rec[c]->p, rec[c]->f, rec[c]->g, m, iso, leftAssoc, N);
        double cubeLo[3], cubeHi[3], x[3];
        for (int a = 0; a < 3; ++a) {
            cubeLo[a] = cl.lo[a] + (double)idx[a] * cl.h[a];
            cubeHi[a] = cl.lo[a] + (double)(idx[a] + 1u) * cl.h[a];
        }
        const uint32_t info = dualSolve(N, m, tau, leftAssoc, cubeLo, cubeHi, x);
        outV[3 * vtx] = x[0], outV[3 * vtx + 1] = x[1], outV[3 * vtx + 2] = x[2];
        if (outI) outI[vtx] = (uint8_t)info;
        ++vtx;
    }
    for (uint64_t e = 0; e < nEdges && T > 0; ++e) {
        if (!interior.test(e)) continue;
        uint32_t L, a, idx[3], Q[4];
        edgeOf(e, L, a, idx);
        dualQuadCubes(idx, a, n, Q);
        uint64_t q[4];
        for (int c = 0; c < 4; ++c) q[c] = mixed.rank(Q[c]);
        if (!(v[L] < iso)) std::swap(q[1], q[3]);  // the lower end is outside: the quad is reversed
        uint64_t* o = outT + 6 * interior.rank(e);
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        o[3] = q[0], o[4] = q[2], o[5] = q[3];
    }
    if (values) std::memcpy(values, v.data(), nPts * sizeof(double));
    if (V > 0) {
        *verts = outV, *tris = outT, *nVerts = V, *nTris = T;
        if (vertInfo) *vertInfo = outI;
        hVerts.p = hTris.p = hInfo.p = nullptr;
    }
    return HPSDF_OK;
}

}  // namespace

// what hpsdf_extract_surface_dual[_block] reject before anything runs, besides the lattice (0: fine)
int dualArgumentError(double tau, uint32_t flags) {
    if (flags != 0u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_extract_surface_dual: flags must be 0");
    if (!(tau >= 0.0 && tau < 1.0)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_extract_surface_dual: tau must be finite with 0 <= tau < 1");
    return HPSDF_OK;
}

}  // namespace hpsdf

// ExtractSurfaceDual from a serialised block, on the calling thread (no device; the process-wide reduction order)
extern "C" int hpsdf_extract_surface_dual_block(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3],
                                                double iso, double tau, uint32_t flags, double** verts, uint64_t* n_verts, uint64_t** tris,
                                                uint64_t* n_tris, uint8_t** vert_info, double* values) {
    using namespace hpsdf;
    HPSDF_TRY
    if (!lo || !hi || !n || !verts || !n_verts || !tris || !n_tris) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *verts = nullptr, *tris = nullptr, *n_verts = 0, *n_tris = 0;
    if (vert_info) *vert_info = nullptr;
    if (const int rc = dualArgumentError(tau, flags)) return rc;
    hpsdf_tree t;
    int left;
    if (const int rc = treeFromBlock(block, size, t, left)) return rc;
    CheckedLattice cl{};
    if (const int rc = checkLattice("hpsdf_extract_surface_dual_block", kDenseLimits, t.dev.rootCentre, t.dev.rootInvSizes, lo, hi, n, iso, &cl))
        return rc;
    return hostExtractSurfaceDual(t, cl, iso, tau, left, verts, n_verts, tris, n_tris, vert_info, values);
    HPSDF_CATCH
}

// QueryGradient from a serialised block, on the calling thread: no device, no context; treeFromBlock makes the tree the rows are
// answered from.
extern "C" int hpsdf_query_true_gradient_block(const void* block, size_t size, const double* xyz, size_t n, uint32_t flags, double* out,
                                               double* grad) {
    using namespace hpsdf;
    HPSDF_TRY
    if (flags & ~HPSDF_GRADIENT_UNIT) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_query_true_gradient: unknown flag bits");
    if (n && (!xyz || !grad)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    hpsdf_tree t;
    int left;
    if (const int rc = treeFromBlock(block, size, t, left)) return rc;
    hostTrueGradientRows(t, xyz, n, flags, left, out, grad);
    return HPSDF_OK;
    HPSDF_CATCH
}

// QueryHessian from a serialised block, on the calling thread (no device; the process-wide reduction order)
extern "C" int hpsdf_query_hessian_block(const void* block, size_t size, const double* xyz, size_t n, uint32_t flags, double* out, double* grad,
                                         double* hess, double* curv) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = hessianArgumentError(flags, xyz, n, hess, curv)) return rc;
    hpsdf_tree t;
    int left;
    if (const int rc = treeFromBlock(block, size, t, left)) return rc;
    hostHessianRows(t, xyz, n, flags, left, out, grad, hess, curv);
    return HPSDF_OK;
    HPSDF_CATCH
}

// ProjectToSurface from a serialised block, on the calling thread (no device; the process-wide reduction order)
extern "C" int hpsdf_project_block(const void* block, size_t size, const double* xyz, size_t n, double iso, double tol, uint32_t max_iter,
                                   uint32_t flags, double* out_xyz, double* out_val, double* out_grad, uint8_t* out_iters,
                                   uint8_t* out_status) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = projectArgumentError(flags, iso, tol, max_iter)) return rc;
    if (n && (!xyz || !out_xyz)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    hpsdf_tree t;
    int left;
    if (const int rc = treeFromBlock(block, size, t, left)) return rc;
    hostProjectRows(t, xyz, n, iso, tol, max_iter, flags, left, out_xyz, out_val, out_grad, out_iters, out_status);
    return HPSDF_OK;
    HPSDF_CATCH
}

// CastRays from a serialised block, on the calling thread (no device; the process-wide reduction order)
extern "C" int hpsdf_cast_rays_block(const void* block, size_t size, const double* origins, const double* dirs, const double* t_max, size_t n,
                                     double iso, double tol, uint32_t max_iter, uint32_t max_cells, uint32_t flags, uint8_t* out_status,
                                     double* out_t, double* out_xyz, double* out_val, double* out_grad, uint16_t* out_evals,
                                     uint16_t* out_cells) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = castArgumentError(flags, iso, tol, max_iter, max_cells, n, origins, dirs, t_max, out_status)) return rc;
    hpsdf_tree t;
    int left;
    if (const int rc = treeFromBlock(block, size, t, left)) return rc;
    hostCastRows(t, origins, dirs, t_max, n, CastArgs{iso, tol, max_iter, max_cells, flags, 0u}, left, out_status, out_t, out_xyz, out_val, out_grad,
                 out_evals, out_cells);
    return HPSDF_OK;
    HPSDF_CATCH
}

// QueryBounds from a serialised block, on the calling thread (no device): the leaves' constants come from leafBound on the host, the
// statements of leaf_consts_kernel
extern "C" int hpsdf_query_bounds_block(const void* block, size_t size, const double* boxes, size_t n, uint32_t subdiv, uint32_t max_leaves,
                                        double* out_lo, double* out_hi, uint8_t* out_status, uint32_t* out_leaves) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = boundsArgumentError(subdiv, max_leaves, n, boxes, out_lo, out_hi, out_status)) return rc;
    HostTree ht;
    if (const int rc = parseBlock(block, size, &ht)) return rc;
    hostBoundsRows(ht.view, boxes, nullptr, n, subdiv, max_leaves, out_lo, out_hi, out_status, out_leaves);
    return HPSDF_OK;
    HPSDF_CATCH
}

extern "C" int hpsdf_query_bounds_grid_block(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3],
                                             uint32_t subdiv, uint32_t max_leaves, double* out_lo, double* out_hi, uint8_t* out_status,
                                             uint32_t* out_leaves) {
    using namespace hpsdf;
    HPSDF_TRY
    if (!lo || !hi || !n) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = boundsArgumentError(subdiv, max_leaves, 1, lo, out_lo, out_hi, out_status)) return rc;
    HostTree ht;
    if (const int rc = parseBlock(block, size, &ht)) return rc;
    BoxGrid g{};
    size_t count = 0;
    if (const int rc = checkBoundsGrid("hpsdf_query_bounds_grid_block", ht.view.rootCentre, ht.view.rootInvSizes, lo, hi, n, &g, &count)) return rc;
    hostBoundsRows(ht.view, nullptr, &g, count, subdiv, max_leaves, out_lo, out_hi, out_status, out_leaves);
    return HPSDF_OK;
    HPSDF_CATCH
}

// Integrate from a serialised block, on the calling thread (no device): list 0 from the mirror's records, the leaves' constants from
// leafBound on the host
extern "C" int hpsdf_integrate_block(const void* block, size_t size, double iso, uint32_t depth, uint32_t samples, uint32_t max_cells,
                                     hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = integrateArgumentError(iso, depth, samples, max_cells, out, out_cells, out_n_cells)) return rc;
    HostTree ht;
    if (const int rc = parseBlock(block, size, &ht)) return rc;
    const IntegrateArgs a{iso, depth, samples, max_cells};
    return hostIntegrate(ht.view, ht.m.recs.size(), a, out, out_cells, out_n_cells);
    HPSDF_CATCH
}
