// The vertex of a crossing lattice edge (include/hpsdf.h, "ExtractSurface"): one set of statements for the marching-cubes calls
// (surface_common.hpp), for dual contouring's Hermite samples on the device (surface_dual.hip) and on the calling thread
// (host_query.cpp).  No HIP beyond the function attributes: the device-free units include it too.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hpsdf {

namespace {

// The vertex on the edge from lattice point idx = (i, j, k) along axis a, whose ends hold va and vb.  Both calls' vertices are these
// statements in this order; no multiply-add is fused (the build's -ffp-contract=off).
__host__ __device__ __forceinline__ void edgeVertex(const double* lo, const double* h, const uint32_t (&idx)[3], uint32_t a, double va, double vb,
                                                    double iso, double (&p)[3]) {
    const double t = (iso - va) / (vb - va);
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = lo[d] + (double)idx[d] * h[d];
    const double xb = lo[a] + (double)(idx[a] + 1u) * h[a];
    p[a] = p[a] + t * (xb - p[a]);
}

}  // namespace

}  // namespace hpsdf
