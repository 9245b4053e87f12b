// CastRays: the first crossing of each ray with the level set {Query = iso} (include/hpsdf.h, "CastRays"; the walk's statements are
// ray_cast.hpp's castRay, the field evaluation is QueryGradient's trueGradientPoint, jet_point.hpp).
//
// One lane per ray: 56 bytes read (origin, direction, t_max), 1 written, plus whichever of the optional outputs are asked for
// (8 + 24 + 8 + 24 + 2 + 2), plus one leaf's row per field evaluation and one descent (8-byte records) per leaf visited.
//   cast_rays_kernel<MAXP>      any tree, grid-stride in workgroups of 256.  A lane walks until its ray stops; lanes that have stopped
//                               idle until the last lane of their wave has: a wave costs its slowest ray's evaluations.  (No refill of
//                               idle lanes and no cooperative traversal.)  The walk has one call of the field evaluation whatever
//                               its phase, so the unrolled leaf code exists once per kernel.
//   cast_rays_few_kernel<MAXP>  the same for a handful of rays in workgroups of one wave.
// Every sample goes through the full descent of trueGradientPoint: the leaf the walk holds is not reused for the evaluation, and the
// samples compute the gradient as well as the value (only the refinement and the final row need it).
// The double outputs leave through non-temporal stores like Query's; the byte and 16-bit outputs are plain stores.
//
// Built with -ffp-contract=off like every other unit: the host version (host_query.cpp, hostCastRay) gives the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_types.hpp"
#include "jet_point.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "ray_cast.hpp"

namespace hpsdf {

namespace {

struct CastOut {
    uint8_t* status;  // never null
    double* t;        // the rest may be null
    double* xyz;
    double* val;
    double* grad;
    uint16_t* evals;
    uint16_t* cells;
};

// castRay's Field on the device
template <int MAXP>
struct DeviceCastField {
    const TreeDev& t;
    const double* sNl;
    const double* sRec;
    __device__ __forceinline__ double eval(const double (&x)[3], double (&g)[3]) const {
        return trueGradientPoint<MAXP>(t, x[0], x[1], x[2], false, sNl, sRec, g);
    }
    // trueGradientPoint's descent on a point of the unit cube, through the records alone: the complete levels by comparison, the
    // 8-byte top table, then the nodes
    __device__ __forceinline__ void locate(const double (&pu)[3], double (&lo)[3], double (&hi)[3], int& degree) const {
        double cx = 0.0, cy = 0.0, cz = 0.0, q = 0.25;
        uint32_t ix = 0, iy = 0, iz = 0;
        for (int depth = 0; depth < t.topDepth; ++depth) {
            const bool ux = pu[0] >= cx, uy = pu[1] >= cy, uz = pu[2] >= cz;
            ix = ix * 2u + (ux ? 1u : 0u);
            iy = iy * 2u + (uy ? 1u : 0u);
            iz = iz * 2u + (uz ? 1u : 0u);
            cx = ux ? cx + q : cx - q;
            cy = uy ? cy + q : cy - q;
            cz = uz ? cz + q : cz - q;
            q = q * 0.5;
        }
        const uint32_t code = ix + ((iy + (iz << t.topDepth)) << t.topDepth);
        NodeRec rec = t.topRec[code];
        while (rec.b == kInteriorTag) {
            const bool ux = pu[0] >= cx, uy = pu[1] >= cy, uz = pu[2] >= cz;
            const uint32_t idx = rec.a + (ux ? 1u : 0u) + (uy ? 2u : 0u) + (uz ? 4u : 0u);
            cx = ux ? cx + q : cx - q;
            cy = uy ? cy + q : cy - q;
            cz = uz ? cz + q : cz - q;
            q = q * 0.5;
            rec = t.nodes[idx];
        }
        const double h = q + q;
        lo[0] = cx - h, lo[1] = cy - h, lo[2] = cz - h;
        hi[0] = cx + h, hi[1] = cy + h, hi[2] = cz + h;
        degree = (int)rec.b;
    }
};

template <int MAXP>
__device__ __forceinline__ void castOne(const TreeDev& t, const double* origins, const double* dirs, const double* tMax, size_t i,
                                        const CastArgs& a, const double* sNl, const double* sRec, CastRow& r) {
    const double o[3] = {origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
    const double d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    DeviceCastField<MAXP> F{t, sNl, sRec};
    castRay(F, t.rootCentre, t.rootInvSizes, t.leftAssoc, o, d, tMax[i], a, r);
}

template <bool NT>
__device__ __forceinline__ void storeCastRow(size_t i, const CastRow& r, const CastOut& o) {
    if (NT) {
        if (o.t != nullptr) __builtin_nontemporal_store(r.t, &o.t[i]);
        if (o.xyz != nullptr) {
            __builtin_nontemporal_store(r.x[0], &o.xyz[3 * i]);
            __builtin_nontemporal_store(r.x[1], &o.xyz[3 * i + 1]);
            __builtin_nontemporal_store(r.x[2], &o.xyz[3 * i + 2]);
        }
        if (o.val != nullptr) __builtin_nontemporal_store(r.f, &o.val[i]);
        if (o.grad != nullptr) {
            __builtin_nontemporal_store(r.g[0], &o.grad[3 * i]);
            __builtin_nontemporal_store(r.g[1], &o.grad[3 * i + 1]);
            __builtin_nontemporal_store(r.g[2], &o.grad[3 * i + 2]);
        }
    } else {
        if (o.t != nullptr) o.t[i] = r.t;
        if (o.xyz != nullptr) o.xyz[3 * i] = r.x[0], o.xyz[3 * i + 1] = r.x[1], o.xyz[3 * i + 2] = r.x[2];
        if (o.val != nullptr) o.val[i] = r.f;
        if (o.grad != nullptr) o.grad[3 * i] = r.g[0], o.grad[3 * i + 1] = r.g[1], o.grad[3 * i + 2] = r.g[2];
    }
    o.status[i] = (uint8_t)r.status;
    if (o.evals != nullptr) o.evals[i] = (uint16_t)(r.evals > 65535u ? 65535u : r.evals);
    if (o.cells != nullptr) o.cells[i] = (uint16_t)(r.cells > 65535u ? 65535u : r.cells);
}

}  // namespace

// Any tree, one lane per ray, grid-stride in workgroups of 256.  No output array may alias an input.
template <int MAXP>
__global__ __launch_bounds__(256) void cast_rays_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ origins,
                                                        const double* __restrict__ dirs, const double* __restrict__ tMax, size_t n, CastArgs a,
                                                        CastOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        CastRow r;
        castOne<MAXP>(t, origins, dirs, tMax, i, a, sNl, sRec, r);
        storeCastRow<true>(i, r, o);
    }
}

// A handful of rays (a small call that reaches the device): one launch of one-wave workgroups, like project_few_kernel.
template <int MAXP>
__global__ __launch_bounds__(64) void cast_rays_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ origins,
                                                           const double* __restrict__ dirs, const double* __restrict__ tMax, uint32_t n,
                                                           CastArgs a, CastOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        CastRow r;
        castOne<MAXP>(t, origins, dirs, tMax, i, a, sNl, sRec, r);
        storeCastRow<false>(i, r, o);
    }
}

// dOutStatus is required; the other outputs may be null.  n < 2^32 is not required: every index is a size_t.
hipError_t launchCastRays(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dOrigins, const double* dDirs,
                          const double* dTMax, size_t n, const CastArgs& a, uint8_t* dOutStatus, double* dOutT, double* dOutXyz, double* dOutVal,
                          double* dOutGrad, uint16_t* dOutEvals, uint16_t* dOutCells) {
    if (n == 0) return hipSuccess;
    const CastOut o{dOutStatus, dOutT, dOutXyz, dOutVal, dOutGrad, dOutEvals, dOutCells};
    const PointLaunch l(n);
    forMaxDegree<2, 3, 5, 12>(t.maxDegree, [&](auto P) {
        constexpr int MAXP = decltype(P)::value;
        if (l.few)
            hipLaunchKernelGGL((cast_rays_few_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dOrigins, dDirs, dTMax, (uint32_t)n, a, o);
        else
            hipLaunchKernelGGL((cast_rays_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dOrigins, dDirs, dTMax, n, a, o);
    });
    return hipGetLastError();
}

}  // namespace hpsdf
