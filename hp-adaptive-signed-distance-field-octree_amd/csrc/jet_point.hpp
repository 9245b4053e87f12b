// One point through the tree on the device, down to the leaf's polynomial with its derivatives: jetPoint<ORDER, MAXP>, the per-point
// routine of the QueryGradient kernels (query_gradient.hip), of the projection, ray and dual-contouring kernels (project.hip,
// cast_rays.hip, surface_dual.hip), which run it once per evaluation, and of the QueryHessian kernels (query_hessian.hip).  The text
// stands once and is instantiated by derivative order, so every kernel holds the straight-line body it would hold with the text
// written out for its order (a routine that takes the leaf's evaluation as an argument, or a descent that fills a struct, changed the
// kernels' register allocation).  Query's own queryPoint (order 0) stays in leaf_eval.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_types.hpp"
#include "leaf_eval.hpp"
#include "leaf_jet.hpp"

namespace hpsdf {

__device__ __forceinline__ double quietNaN() { return __longlong_as_double(0x7FF8000000000000ll); }

template <int ORDER>
using CurvOut = std::conditional_t<(ORDER >= 2), double (&)[2], NoOutput>;

// queryPoint's statements (leaf_eval.hpp) down to the leaf, then leafJet<ORDER> (leaf_jet.hpp; include/hpsdf.h, "QueryGradient" and
// "QueryHessian").  ORDER 1: the value and the world gradient, normalised under unit.  ORDER 2 adds the world Hessian (xx, yy, zz, xy,
// xz, yz) and, if wanted, the level set's (mean, gauss) curvature from the gradient before its normalisation.  Outside the root, or
// with a NaN coordinate: DBL_MAX and quiet NaNs.
template <int ORDER, int MAXP>
__device__ __forceinline__ double jetPoint(const TreeDev& t, double x, double y, double z, bool unit, bool wantCurv, const double* sNl,
                                           const double* sRec, double (&g)[3], HessOut<ORDER> H, CurvOut<ORDER> curv) {
    static_assert(ORDER == 1 || ORDER == 2, "order 0 is queryPoint");
    // Octree.cpp:665
    const double px = (x - t.rootCentre[0]) * t.rootInvSizes[0];
    const double py = (y - t.rootCentre[1]) * t.rootInvSizes[1];
    const double pz = (z - t.rootCentre[2]) * t.rootInvSizes[2];
    // :668 containment on the f32 cast, both ends inclusive; NaN fails
    const float fx = (float)px, fy = (float)py, fz = (float)pz;
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) {
        g[0] = g[1] = g[2] = quietNaN();
        if constexpr (ORDER >= 2) {
            H[0] = H[1] = H[2] = H[3] = H[4] = H[5] = quietNaN();
            curv[0] = curv[1] = quietNaN();
        }
        return DBL_MAX;
    }
    // :674-701, the complete levels by comparison alone (>= takes the upper child), then one table lookup
    double cx = 0.0, cy = 0.0, cz = 0.0, q = 0.25;
    uint32_t ix = 0, iy = 0, iz = 0;
    int depth = 0;
    for (; depth < t.topDepth; ++depth) {
        const bool ux = px >= cx, uy = py >= cy, uz = pz >= cz;
        ix = ix * 2u + (ux ? 1u : 0u);
        iy = iy * 2u + (uy ? 1u : 0u);
        iz = iz * 2u + (uz ? 1u : 0u);
        cx = ux ? cx + q : cx - q;
        cy = uy ? cy + q : cy - q;
        cz = uz ? cz + q : cz - q;
        q = q * 0.5;
    }
    const uint32_t code = ix + ((iy + (iz << t.topDepth)) << t.topDepth);
    // the top entry's line: the record and, for a leaf of degree <= 2, its coefficients (issued together)
    const TopEntry* __restrict__ e = t.top + code;
    const uint2 hdr = *reinterpret_cast<const uint2*>(e);
    double cv[10];
    {
        const double2* __restrict__ c2 = reinterpret_cast<const double2*>(e->c);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double2 v = c2[i];
            cv[2 * i] = v.x;
            cv[2 * i + 1] = v.y;
        }
    }
    NodeRec rec{hdr.x, hdr.y};
    double f, gu[3], hu[6];
    if (rec.b <= 2u) {
        const double s = (double)(2 << depth);  // :862
        const double u[3] = {(px - cx) * s, (py - cy) * s, (pz - cz) * s};
        if (rec.b == 2u)
            f = leafJetVals<ORDER, 2>(cv, u, depth, sNl, sRec, gu, hessOut<ORDER>(hu));
        else if (rec.b == 1u)
            f = leafJetVals<ORDER, 1>(cv, u, depth, sNl, sRec, gu, hessOut<ORDER>(hu));
        else
            f = leafJetVals<ORDER, 0>(cv, u, depth, sNl, sRec, gu, hessOut<ORDER>(hu));
    } else {
        while (rec.b == kInteriorTag) {
            const bool ux = px >= cx, uy = py >= cy, uz = pz >= cz;
            const uint32_t idx = rec.a + (ux ? 1u : 0u) + (uy ? 2u : 0u) + (uz ? 4u : 0u);
            cx = ux ? cx + q : cx - q;
            cy = uy ? cy + q : cy - q;
            cz = uz ? cz + q : cz - q;
            q = q * 0.5;
            ++depth;
            rec = t.nodes[idx];
        }
        const double s = (double)(2 << depth);  // :862
        const double u[3] = {(px - cx) * s, (py - cy) * s, (pz - cz) * s};
        f = leafJetOf<ORDER, MAXP>(t.coeffs + rec.a, (int)rec.b, u, depth, sNl, sRec, gu, hessOut<ORDER>(hu));
    }
    if constexpr (ORDER == 1) {
        finishTrueGradient(gu, depth, t.rootInvSizes, unit, t.leftAssoc, g);
    } else {
        finishTrueGradient(gu, depth, t.rootInvSizes, false, t.leftAssoc, g);
        finishHessian(hu, depth, t.rootInvSizes, H);
        if (wantCurv) levelSetCurvature(g, H, t.leftAssoc, curv);
        if (unit) unitGradient(g, t.leftAssoc);
    }
    return f;
}

template <int MAXP>
__device__ __forceinline__ double trueGradientPoint(const TreeDev& t, double x, double y, double z, bool unit, const double* sNl,
                                                    const double* sRec, double (&g)[3]) {
    return jetPoint<1, MAXP>(t, x, y, z, unit, false, sNl, sRec, g, NoOutput{}, NoOutput{});
}

template <int MAXP>
__device__ __forceinline__ double hessianPoint(const TreeDev& t, double x, double y, double z, bool unit, bool wantCurv, const double* sNl,
                                               const double* sRec, double (&g)[3], double (&H)[6], double (&curv)[2]) {
    return jetPoint<2, MAXP>(t, x, y, z, unit, wantCurv, sNl, sRec, g, H, curv);
}

}  // namespace hpsdf
