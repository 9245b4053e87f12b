// What lets a fit sample any field: an analytic field (field_eval.hpp), a sample array, a mesh (mesh_distance.hpp), each
// optionally under the CSG wrapper around an old tree (leaf_eval.hpp, queryPoint).  Included by fit_kernels.hpp.
#pragma once
#include "field_eval.hpp"
#include "leaf_eval.hpp"
#include "mesh_distance.hpp"

namespace hpsdf {

// the CSG wrapper of Octree.cpp:355-400 around an inner field value v
template <bool CSG>
__device__ __forceinline__ double applyCsg(const FieldDev& f, double v, double x, double y, double z, const double* sNl,
                                           const double* sRec) {
    if constexpr (CSG) {
        const double o = queryPoint<12>(f.oldTree, x, y, z, sNl, sRec);
        switch (f.csgOp) {
            case HPSDF_OP_UNION: v = o < v ? o : v; break;                   // std::min(old, F)
            case HPSDF_OP_SUBTRACT: v = (o * -1.0) < v ? v : (o * -1.0); break;  // std::max(-old, F)
            default: v = o < v ? v : o; break;                               // std::max(old, F)
        }
    }
    return v;
}

// F at a world-space point, with the optional CSG wrapper of Octree.cpp:355-400
template <int KIND, bool CSG, bool LEFT>
__device__ __forceinline__ double fieldEvalWorld(const FieldDev& f, double x, double y, double z, uint64_t sampleIdx,
                                                 const double* sNl, const double* sRec, uint32_t& meshHint) {
    double v;
    if constexpr (KIND == kFieldAnalytic)
        v = analyticEval<LEFT>(f, x, y, z);
    else if constexpr (KIND == kFieldSamples)
        v = f.samples[sampleIdx];
    else  // SURVEY 3.4 user glue: (f64) mesh.SignedDistanceAtPt(p.cast<f32>())
        v = (double)meshSignedDistance(f.mesh, V3{(float)x, (float)y, (float)z}, meshHint);
    return applyCsg<CSG>(f, v, x, y, z, sNl, sRec);
}

}  // namespace hpsdf
