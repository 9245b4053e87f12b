// QueryGradient: the value of a tree at points and the gradient of the polynomial that value comes from (include/hpsdf.h,
// "QueryGradient"; the arithmetic is leaf_jet.hpp's).  QueryWithGradient -- the reference's per-axis shortcut -- stays in kernels.hip.
//
// One lane per point: 24 bytes read, 8 + 24 written (non-temporally, as Query's results leave), plus the leaf's row.
//   query_true_gradient_top_kernel   trees whose leaves all sit in the top table with degree <= 2 (what the default thresholds produce):
//                                    the wave fetches the points' 128-byte lines cooperatively into LDS, as query_kernel does;
//   query_true_gradient_kernel<MAXP> any tree: queryPoint's descent (top table, then the walk), the leaf's coefficients lane by lane;
//   query_true_gradient_few_kernel   the same for a handful of points in workgroups of one wave.
// The per-point routine of the last two, trueGradientPoint, is jet_point.hpp's jetPoint at order 1 (project.hip runs it too).
// Rows of points outside the root (or with a NaN coordinate) are DBL_MAX and three quiet NaNs.
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

__device__ __forceinline__ void storeGradientRow(size_t i, double f, const double (&g)[3], double* __restrict__ out, double* __restrict__ grad) {
    if (out != nullptr) __builtin_nontemporal_store(f, &out[i]);
    __builtin_nontemporal_store(g[0], &grad[3 * i]);
    __builtin_nontemporal_store(g[1], &grad[3 * i + 1]);
    __builtin_nontemporal_store(g[2], &grad[3 * i + 2]);
}

}  // namespace

// Any tree, one lane per point, grid-stride in workgroups of 256.
template <int MAXP>
__global__ __launch_bounds__(256) void query_true_gradient_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                                  size_t n, uint32_t flags, double* __restrict__ out, double* __restrict__ grad) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const bool unit = (flags & HPSDF_GRADIENT_UNIT) != 0u;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double g[3];
        const double f = trueGradientPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], unit, sNl, sRec, g);
        storeGradientRow(i, f, g, out, grad);
    }
}

// A handful of points (a scalar call that reaches the device): one launch of one-wave workgroups, like query_few_kernel.
template <int MAXP>
__global__ __launch_bounds__(64) void query_true_gradient_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                                     uint32_t n, uint32_t flags, double* __restrict__ out, double* __restrict__ grad) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) {
        double g[3];
        const double f = trueGradientPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (flags & HPSDF_GRADIENT_UNIT) != 0u, sNl, sRec, g);
        if (out != nullptr) out[i] = f;
        grad[3 * i] = g[0], grad[3 * i + 1] = g[1], grad[3 * i + 2] = g[2];
    }
}

// Trees whose leaves ALL sit in the top table with degree <= 2.  Random points share nothing, so a point costs one 128-byte line out of
// L2; the wave fetches them as query_kernel does (kernels.hip, queryTopBody): in step k the 8 lanes of every group read the consecutive
// 16-byte chunks of the line of the group's k-th point straight into LDS (lane-linear destination, per-lane source), two passes of four
// steps through a 4 KB per-wave window, and every lane reads back its own point's row: [record][c0 c1] .. [c8 c9].
template <int TOPD>
__global__ __launch_bounds__(256) void query_true_gradient_top_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                                      size_t n, uint32_t flags, double* __restrict__ out, double* __restrict__ grad) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ double2 sRows[4][4][66];  // per wave: 4 steps x 64 lanes x 16 B, each kilobyte followed by 32 bytes against bank conflicts
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const bool unit = (flags & HPSDF_GRADIENT_UNIT) != 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane & ~7, sub = lane & 7;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        const size_t i = base + threadIdx.x;
        const bool valid = i < n;
        const size_t il = valid ? i : n - 1;
        const double x = xyz[3 * il], y = xyz[3 * il + 1], z = xyz[3 * il + 2];
        const double p3[3] = {(x - t.rootCentre[0]) * t.rootInvSizes[0], (y - t.rootCentre[1]) * t.rootInvSizes[1],
                              (z - t.rootCentre[2]) * t.rootInvSizes[2]};  // Octree.cpp:665
        const float fx = (float)p3[0], fy = (float)p3[1], fz = (float)p3[2];
        const bool inside = fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f;  // :668
        const int topDepth = TOPD > 0 ? TOPD : t.topDepth;
        int k3[3];
        double c3[3];
        topCell(p3, topDepth, k3, c3);
        uint32_t code = (uint32_t)(k3[0] + ((k3[1] + (k3[2] << topDepth)) << topDepth));
        if (!inside) code = 0;  // any valid line; the row is DBL_MAX and NaNs
        uint32_t ck[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) ck[k] = __shfl(code, grp | k, 64);
        uint2 hdr = make_uint2(0u, 0u);
        double cv[10];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const char* src = reinterpret_cast<const char*>(t.top + ck[pass * 4 + k]) + sub * 16;
                if (sub < 6)  // bytes 96..127 of an entry are padding
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)&sRows[wave][k][0], 16, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if ((sub >> 2) == pass) {
                const double2* row = &sRows[wave][sub & 3][grp];
                hdr = *reinterpret_cast<const uint2*>(row);
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const double2 v = row[1 + c];
                    cv[2 * c] = v.x;
                    cv[2 * c + 1] = v.y;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();  // the window is rewritten by the next pass / tile
        }
        double f = DBL_MAX;
        double g[3] = {quietNaN(), quietNaN(), quietNaN()};
        if (inside) {
            const double s = (double)(2 << topDepth);  // :862
            const double u[3] = {(p3[0] - c3[0]) * s, (p3[1] - c3[1]) * s, (p3[2] - c3[2]) * s};
            double gu[3];
            if (hdr.y == 2u)
                f = leafJetVals<1, 2>(cv, u, topDepth, sNl, sRec, gu, NoOutput{});
            else if (hdr.y == 1u)
                f = leafJetVals<1, 1>(cv, u, topDepth, sNl, sRec, gu, NoOutput{});
            else
                f = leafJetVals<1, 0>(cv, u, topDepth, sNl, sRec, gu, NoOutput{});
            finishTrueGradient(gu, topDepth, t.rootInvSizes, unit, t.leftAssoc, g);
        }
        if (valid) storeGradientRow(i, f, g, out, grad);
    }
}

// dOut may be null (gradients only).  n < 2^32 is not required: every index is a size_t.
hipError_t launchQueryTrueGradient(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dXyz, size_t n,
                                   uint32_t flags, double* dOut, double* dGrad, bool allInline) {
    if (n == 0) return hipSuccess;
    const PointLaunch l(n);
    if (!l.few && allInline) {
        if (t.topDepth == 4)
            hipLaunchKernelGGL((query_true_gradient_top_kernel<4>), l.grid, l.block, 0, stream, t, dTables, dXyz, n, flags, dOut, dGrad);
        else
            hipLaunchKernelGGL((query_true_gradient_top_kernel<0>), l.grid, l.block, 0, stream, t, dTables, dXyz, n, flags, dOut, dGrad);
        return hipGetLastError();
    }
    forMaxDegree<2, 3, 5, 12>(t.maxDegree, [&](auto P) {
        constexpr int MAXP = decltype(P)::value;
        if (l.few)
            hipLaunchKernelGGL((query_true_gradient_few_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, (uint32_t)n, flags, dOut, dGrad);
        else
            hipLaunchKernelGGL((query_true_gradient_kernel<MAXP>), l.grid, l.block, 0, stream, t, dTables, dXyz, n, flags, dOut, dGrad);
    });
    return hipGetLastError();
}

}  // namespace hpsdf
