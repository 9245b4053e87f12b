// QueryHessian: the value of a tree at points, the gradient and the second derivative of the polynomial that value comes from, and the
// mean and Gaussian curvature of its level set (include/hpsdf.h, "QueryHessian"; the arithmetic is leaf_jet.hpp's).
//
// One lane per point: 24 bytes read, up to 8 + 24 + 48 + 16 written (non-temporally, and only the outputs asked for), plus the leaf's row.
//   query_hessian_kernel<MAXP>       any tree: hessianPoint's descent (top table, then the walk), the leaf's coefficients lane by lane;
//   query_hessian_few_kernel<MAXP>   the same for a handful of points in workgroups of one wave.
// There is no cooperative-fetch kernel for trees that sit in the top table: their leaves have degree <= 2, a constant Hessian at best,
// and the any-tree kernel reads their coefficients from the top entry's own line already.
// Rows of points outside the root (or with a NaN coordinate) are DBL_MAX and quiet NaNs.
//
// Built with -ffp-contract=off like every other unit: the host versions (host_query.cpp) give the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_types.hpp"
#include "jet_point.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"

namespace hpsdf {

namespace {

struct HessianOut {
    double* __restrict__ out;   // [n]     may be null
    double* __restrict__ grad;  // [n, 3]  may be null
    double* __restrict__ hess;  // [n, 6]  may be null
    double* __restrict__ curv;  // [n, 2]  may be null
};

__device__ __forceinline__ void storeHessianRow(size_t i, double f, const double (&g)[3], const double (&H)[6], const double (&curv)[2],
                                                const HessianOut& o) {
    if (o.out != nullptr) __builtin_nontemporal_store(f, &o.out[i]);
    if (o.grad != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(g[k], &o.grad[3 * i + k]);
    }
    if (o.hess != nullptr) {
#pragma unroll
        for (int k = 0; k < 6; ++k) __builtin_nontemporal_store(H[k], &o.hess[6 * i + k]);
    }
    if (o.curv != nullptr) {
        __builtin_nontemporal_store(curv[0], &o.curv[2 * i]);
        __builtin_nontemporal_store(curv[1], &o.curv[2 * i + 1]);
    }
}

}  // namespace

// Any tree, one lane per point, grid-stride in workgroups of 256.
template <int MAXP>
__global__ __launch_bounds__(256) void query_hessian_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz, size_t n,
                                                            uint32_t flags, HessianOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const bool unit = (flags & HPSDF_GRADIENT_UNIT) != 0u, wantCurv = o.curv != nullptr;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double g[3], H[6], curv[2] = {0.0, 0.0};
        const double f = hessianPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], unit, wantCurv, sNl, sRec, g, H, curv);
        storeHessianRow(i, f, g, H, curv, o);
    }
}

// A handful of points (a scalar call that reaches the device): one launch of one-wave workgroups, like query_few_kernel.
template <int MAXP>
__global__ __launch_bounds__(64) void query_hessian_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                               uint32_t n, uint32_t flags, HessianOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        double g[3], H[6], curv[2] = {0.0, 0.0};
        const double f = hessianPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (flags & HPSDF_GRADIENT_UNIT) != 0u, o.curv != nullptr,
                                            sNl, sRec, g, H, curv);
        storeHessianRow(i, f, g, H, curv, o);
    }
}

// Every output may be null.  n < 2^32 is not required: every index is a size_t.
hipError_t launchQueryHessian(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dXyz, size_t n, uint32_t flags,
                              double* dOut, double* dGrad, double* dHess, double* dCurv) {
    if (n == 0) return hipSuccess;
    const HessianOut o{dOut, dGrad, dHess, dCurv};
    const PointLaunch l(n);
    forMaxDegree<2, 3, 5, 12>(t.maxDegree, [&](auto P) {
        constexpr int MAXP = decltype(P)::value;
        if (l.few)
            hipLaunchKernelGGL((query_hessian_few_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, (uint32_t)n, flags, o);
        else
            hipLaunchKernelGGL((query_hessian_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, n, flags, o);
    });
    return hipGetLastError();
}

}  // namespace hpsdf
