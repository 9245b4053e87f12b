// ProjectToSurface: Newton's iteration x <- x - (f(x) - iso) grad f(x) / |grad f(x)|^2 onto the level set {Query = iso}, run to a
// tolerance on the device (include/hpsdf.h, "ProjectToSurface"; the loop's statements are leaf_jet.hpp's projectStep, the field
// evaluation is QueryGradient's trueGradientPoint, jet_point.hpp).
//
// One lane per point: 24 bytes read, 24 written, plus whichever of the optional outputs are asked for (8 + 24 + 1 + 1), plus one leaf's
// row per field evaluation.
//   project_kernel<MAXP>      any tree, grid-stride in workgroups of 256.  A lane loops until its point stops; lanes that have stopped
//                             idle until the last lane of their wave has: a wave costs its slowest point's evaluations.  (No refill of
//                             idle lanes, and no cooperative fetch of the top table's lines as query_true_gradient_top_kernel does it --
//                             the positions change every step; trees of that shape run project_kernel<2>.)
//   project_few_kernel<MAXP>  the same for a handful of points in workgroups of one wave.
// The double outputs leave through non-temporal stores like Query's; the two byte outputs are plain stores.
//
// Built with -ffp-contract=off like every other unit: the host version (host_query.cpp, hostProjectPoint) gives the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_types.hpp"
#include "jet_point.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"

namespace hpsdf {

namespace {

struct ProjectOut {
    double* xyz;      // never null
    double* val;      // the rest may be null
    double* grad;
    uint8_t* iters;
    uint8_t* status;
};

// the loop of include/hpsdf.h for one point; x: the point on entry, where the loop stopped on return
template <int MAXP>
__device__ __forceinline__ void projectPoint(const TreeDev& t, double (&x)[3], const ProjectArgs& a, const double* sNl, const double* sRec,
                                             double& f, double (&g)[3], uint32_t& k, int& status) {
    k = 0;
    for (;;) {
        f = trueGradientPoint<MAXP>(t, x[0], x[1], x[2], false, sNl, sRec, g);
        status = projectStep(f, g, a.iso, a.tol, k, a.maxIter, t.leftAssoc, x);
        if (status >= 0) break;
        ++k;
    }
    if ((a.flags & HPSDF_PROJECT_UNIT) != 0u) unitGradient(g, t.leftAssoc);  // (status 2: the row is NaN and stays NaN)
}

template <bool NT>
__device__ __forceinline__ void storeProjectRow(size_t i, const double (&x)[3], double f, const double (&g)[3], uint32_t k, int status,
                                                const ProjectOut& o) {
    if (NT) {
        __builtin_nontemporal_store(x[0], &o.xyz[3 * i]);
        __builtin_nontemporal_store(x[1], &o.xyz[3 * i + 1]);
        __builtin_nontemporal_store(x[2], &o.xyz[3 * i + 2]);
        if (o.val != nullptr) __builtin_nontemporal_store(f, &o.val[i]);
        if (o.grad != nullptr) {
            __builtin_nontemporal_store(g[0], &o.grad[3 * i]);
            __builtin_nontemporal_store(g[1], &o.grad[3 * i + 1]);
            __builtin_nontemporal_store(g[2], &o.grad[3 * i + 2]);
        }
    } else {
        o.xyz[3 * i] = x[0], o.xyz[3 * i + 1] = x[1], o.xyz[3 * i + 2] = x[2];
        if (o.val != nullptr) o.val[i] = f;
        if (o.grad != nullptr) o.grad[3 * i] = g[0], o.grad[3 * i + 1] = g[1], o.grad[3 * i + 2] = g[2];
    }
    if (o.iters != nullptr) o.iters[i] = (uint8_t)k;
    if (o.status != nullptr) o.status[i] = (uint8_t)status;
}

}  // namespace

// Any tree, one lane per point, grid-stride in workgroups of 256.  xyz and o.xyz may be the same array: a lane reads its point before
// it writes it, and no lane touches another's row.
template <int MAXP>
__global__ __launch_bounds__(256) void project_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* xyz, size_t n, ProjectArgs a,
                                                      ProjectOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, f, g[3];
        uint32_t k;
        int status;
        projectPoint<MAXP>(t, x, a, sNl, sRec, f, g, k, status);
        storeProjectRow<true>(i, x, f, g, k, status, o);
    }
}

// A handful of points (a scalar call that reaches the device): one launch of one-wave workgroups, like query_true_gradient_few_kernel.
template <int MAXP>
__global__ __launch_bounds__(64) void project_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* xyz, uint32_t n,
                                                         ProjectArgs a, ProjectOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        double x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, f, g[3];
        uint32_t k;
        int status;
        projectPoint<MAXP>(t, x, a, sNl, sRec, f, g, k, status);
        storeProjectRow<false>(i, x, f, g, k, status, o);
    }
}

// dOutXyz may be dXyz; dOutVal, dOutGrad, dOutIters, dOutStatus may be null.  n < 2^32 is not required: every index is a size_t.
hipError_t launchProject(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dXyz, size_t n, const ProjectArgs& a,
                         double* dOutXyz, double* dOutVal, double* dOutGrad, uint8_t* dOutIters, uint8_t* dOutStatus) {
    if (n == 0) return hipSuccess;
    const ProjectOut o{dOutXyz, dOutVal, dOutGrad, dOutIters, dOutStatus};
    const PointLaunch l(n);
    forMaxDegree<2, 3, 5, 12>(t.maxDegree, [&](auto P) {
        constexpr int MAXP = decltype(P)::value;
        if (l.few)
            hipLaunchKernelGGL((project_few_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, (uint32_t)n, a, o);
        else
            hipLaunchKernelGGL((project_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, n, a, o);
    });
    return hipGetLastError();
}

}  // namespace hpsdf
