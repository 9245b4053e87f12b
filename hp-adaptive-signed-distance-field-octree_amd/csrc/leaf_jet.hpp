// A leaf's polynomial with its derivatives -- the value, the gradient and the second derivative of what Query evaluates, not the
// reference's shortcut (FApproxWithGradient, Octree.cpp:904-985, kept as it is in leaf_eval.hpp's evalLeafGradVals) -- as include/hpsdf.h
// states them under "QueryGradient" and "QueryHessian":
//   L_j(u_a)   Query's recurrence (Octree.cpp:876-885), D_0 = 0, D_1 = 1, D_j = D_{j-2} + (2j-1) L_{j-1} (= L_j'),
//              E_0 = E_1 = 0, E_j = E_{j-2} + (2j-1) D_{j-1} (= L_j'');  LN_j = L_j nl[j][d], DN_j = D_j nl[j][d], EN_j = E_j nl[j][d];
//   f          Query's running sum; gu_0 += c_r ((DN_a(x) LN_b(y)) LN_c(z)), gu_1 += c_r ((LN_a DN_b) LN_c), gu_2 += c_r ((LN_a LN_b) DN_c);
//   hu_xx += c_r ((EN_a LN_b) LN_c), hu_yy += c_r ((LN_a EN_b) LN_c), hu_zz += c_r ((LN_a LN_b) EN_c),
//   hu_xy += c_r ((DN_a DN_b) LN_c), hu_xz += c_r ((DN_a LN_b) DN_c), hu_yz += c_r ((LN_a DN_b) DN_c);
//   g_a = (gu_a (double)(2 << d)) rootInvSizes[a]; HPSDF_GRADIENT_UNIT: z = sum3(g^2) in the context's order, g_a / sqrt(z) if z > 0;
//   H_ab = (((hu_ab s) s) rootInvSizes[a]) rootInvSizes[b], s = (double)(2 << d); stored xx, yy, zz, xy, xz, yz;
//   curv = (mean, gauss) of the level set through the point, from the un-normalised world gradient and H.
// The statements stand once, in leafJet<ORDER>: ORDER 0 is f alone, 1 adds gu, 2 adds hu, and a higher order computes the lower ones with
// the lower order's statements in their order (the same bits).  The degree is a run-time int on the calling thread (host_query.cpp) and in
// the kernels' out-of-line any-degree routine, and a compile-time constant in the kernels' unrolled classes (the second half of this file:
// the coefficients and every table entry a register).  Everything is built with -ffp-contract=off, so all of them give the same bits.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

namespace hpsdf {

// Eigen's 3-vector reduction in the context's order (field_eval.hpp's sum3<LEFT> is the same with the order a template parameter)
__host__ __device__ inline double sum3(double a, double b, double c, int leftAssoc) { return leftAssoc ? (a + b) + c : a + (b + c); }

// leafJet's degree: AnyDegree{p} at run time (tables of 13 rows), FixedDegree<P> at compile time (P + 1 rows).  leafJet asks for its
// loops over the degree and the basis rows to be unrolled IN FULL: with a FixedDegree they are, and every table entry is a register;
// with an AnyDegree the request cannot be met and the loops compile as they do without one (build.py turns the compiler's remark about
// that off for the units that include this header).  A plain `#pragma unroll` there, or an unroll count of 1, is honoured -- run-time unrolling, or no peeling -- and changed
// the any-degree routines (profiles/leaf_jet_timing.txt).
struct AnyDegree {
    int p;
    static constexpr int kRows = 13;
    constexpr operator int() const { return p; }
};
template <int P>
struct FixedDegree {
    static constexpr int kRows = P + 1;
    constexpr operator int() const { return P; }
};

// the place of an output that the order leaves out: empty, written NoOutput{} at the call, and no part of the call's machine code
struct NoOutput {};
template <int ORDER>
using GradOut = std::conditional_t<(ORDER >= 1), double (&)[3], NoOutput>;
template <int ORDER>
using HessOut = std::conditional_t<(ORDER >= 2), double (&)[6], NoOutput>;
// hu where the order has second partials, NoOutput{} where it has not
template <int ORDER>
__host__ __device__ inline HessOut<ORDER> hessOut(double (&hu)[6]) {
    if constexpr (ORDER >= 2) return hu;
    else return NoOutput{};
}

// co: the leaf's coefficients in basis order (a pointer, or an array in registers), nc of them; nl: [13][11] normalisation table, rec:
// [13][2] recurrence constants (flat); bidx(r, k): index k of basis row r.  Returns f, leaves the unit-space first partials in gu
// (ORDER >= 1) and the second in hu (ORDER 2).
template <int ORDER, class Degree, class Coeffs, class BasisAt>
__host__ __device__ __attribute__((always_inline)) inline double leafJet(const Coeffs& co, Degree degree, int nc, const double (&u)[3], int depth,
                                                                          const double* nl, const double* rec, BasisAt bidx, GradOut<ORDER> gu,
                                                                          HessOut<ORDER> hu) {
    static_assert(ORDER >= 0 && ORDER <= 2, "value, gradient, second derivative");
    constexpr int R = Degree::kRows;
    double LN[3][R], DN[3][ORDER >= 1 ? R : 1], EN[3][ORDER >= 2 ? R : 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        LN[a][0] = nl[depth];
        if constexpr (ORDER >= 1) DN[a][0] = 0.0 * nl[depth];
        if constexpr (ORDER >= 2) EN[a][0] = 0.0 * nl[depth];
        double m2 = 0.0, m1 = 1.0, d2 = 0.0, d1 = 0.0, e2 = 0.0, e1 = 0.0;  // L, D, E of j-2 and j-1
#pragma clang loop unroll(full)
        for (int j = 1; j <= degree; ++j) {
            const double n = nl[j * 11 + depth];
            const double l = rec[2 * j] * u[a] * m1 - rec[2 * j + 1] * m2;
            double d = 0.0, e = 0.0;
            if constexpr (ORDER >= 1) d = j == 1 ? 1.0 : d2 + (double)(2 * j - 1) * m1;
            if constexpr (ORDER >= 2) e = j == 1 ? 0.0 : e2 + (double)(2 * j - 1) * d1;
            m2 = m1, m1 = l, d2 = d1, d1 = d, e2 = e1, e1 = e;
            LN[a][j] = l * n;
            if constexpr (ORDER >= 1) DN[a][j] = d * n;
            if constexpr (ORDER >= 2) EN[a][j] = e * n;
        }
    }
    double f = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, hxx = 0.0, hyy = 0.0, hzz = 0.0, hxy = 0.0, hxz = 0.0, hyz = 0.0;
#pragma clang loop unroll(full)
    for (int r = 0; r < nc; ++r) {
        const int a = bidx(r, 0), b = bidx(r, 1), c = bidx(r, 2);
        double lp = LN[0][a];
        lp = lp * LN[1][b];
        lp = lp * LN[2][c];
        f = f + co[r] * lp;
        if constexpr (ORDER >= 1) {
            g0 = g0 + co[r] * ((DN[0][a] * LN[1][b]) * LN[2][c]);
            g1 = g1 + co[r] * ((LN[0][a] * DN[1][b]) * LN[2][c]);
            g2 = g2 + co[r] * ((LN[0][a] * LN[1][b]) * DN[2][c]);
        }
        if constexpr (ORDER >= 2) {
            hxx = hxx + co[r] * ((EN[0][a] * LN[1][b]) * LN[2][c]);
            hyy = hyy + co[r] * ((LN[0][a] * EN[1][b]) * LN[2][c]);
            hzz = hzz + co[r] * ((LN[0][a] * LN[1][b]) * EN[2][c]);
            hxy = hxy + co[r] * ((DN[0][a] * DN[1][b]) * LN[2][c]);
            hxz = hxz + co[r] * ((DN[0][a] * LN[1][b]) * DN[2][c]);
            hyz = hyz + co[r] * ((LN[0][a] * DN[1][b]) * DN[2][c]);
        }
    }
    if constexpr (ORDER >= 1) gu[0] = g0, gu[1] = g1, gu[2] = g2;
    if constexpr (ORDER >= 2) hu[0] = hxx, hu[1] = hyy, hu[2] = hzz, hu[3] = hxy, hu[4] = hxz, hu[5] = hyz;
    return f;
}

// g / |g| with |g|^2 = sum3(g^2) in the context's order; a zero (or NaN) vector stays as it is
__host__ __device__ inline void unitGradient(double (&g)[3], int leftAssoc) {
    const double z = sum3(g[0] * g[0], g[1] * g[1], g[2] * g[2], leftAssoc);
    if (z > 0.0) {
        const double nrm = sqrt(z);
        g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
    }
}

// unit-space partials -> world gradient (the chain rule through Octree.cpp:862 and :665), normalised under HPSDF_GRADIENT_UNIT
__host__ __device__ inline void finishTrueGradient(const double (&gu)[3], int depth, const double* rootInvSizes, bool unit, int leftAssoc,
                                                   double (&g)[3]) {
    const double s = (double)(2 << depth);
    g[0] = (gu[0] * s) * rootInvSizes[0];
    g[1] = (gu[1] * s) * rootInvSizes[1];
    g[2] = (gu[2] * s) * rootInvSizes[2];
    if (unit) unitGradient(g, leftAssoc);
}

// unit-space second partials -> world Hessian (the chain rule through Octree.cpp:862 and :665, twice): xx, yy, zz, xy, xz, yz
__host__ __device__ inline void finishHessian(const double (&hu)[6], int depth, const double* rootInvSizes, double (&H)[6]) {
    const double s = (double)(2 << depth);
    H[0] = (((hu[0] * s) * s) * rootInvSizes[0]) * rootInvSizes[0];
    H[1] = (((hu[1] * s) * s) * rootInvSizes[1]) * rootInvSizes[1];
    H[2] = (((hu[2] * s) * s) * rootInvSizes[2]) * rootInvSizes[2];
    H[3] = (((hu[3] * s) * s) * rootInvSizes[0]) * rootInvSizes[1];
    H[4] = (((hu[4] * s) * s) * rootInvSizes[0]) * rootInvSizes[2];
    H[5] = (((hu[5] * s) * s) * rootInvSizes[1]) * rootInvSizes[2];
}

// Mean and Gaussian curvature of the level set through the point, from the world gradient (NOT normalised) and the world Hessian:
// mean = (|g|^2 tr H - g.Hg) / (2 |g|^3), gauss = g.adj(H)g / |g|^4; a field positive outside gives a sphere of radius r (1/r, 1/r^2).
// A zero (or NaN) gradient: two quiet NaNs.
__host__ __device__ inline void levelSetCurvature(const double (&g)[3], const double (&H)[6], int leftAssoc, double (&curv)[2]) {
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    const double Hxx = H[0], Hyy = H[1], Hzz = H[2], Hxy = H[3], Hxz = H[4], Hyz = H[5];
    const double z = sum3(g0 * g0, g1 * g1, g2 * g2, leftAssoc);
    if (!(z > 0.0)) {
        curv[0] = curv[1] = __builtin_nan("");
        return;
    }
    const double Hg0 = sum3(Hxx * g0, Hxy * g1, Hxz * g2, leftAssoc);
    const double Hg1 = sum3(Hxy * g0, Hyy * g1, Hyz * g2, leftAssoc);
    const double Hg2 = sum3(Hxz * g0, Hyz * g1, Hzz * g2, leftAssoc);
    const double q = sum3(g0 * Hg0, g1 * Hg1, g2 * Hg2, leftAssoc);
    const double tr = sum3(Hxx, Hyy, Hzz, leftAssoc);
    curv[0] = (z * tr - q) / ((2.0 * z) * sqrt(z));
    const double A00 = Hyy * Hzz - Hyz * Hyz;
    const double A11 = Hxx * Hzz - Hxz * Hxz;
    const double A22 = Hxx * Hyy - Hxy * Hxy;
    const double A01 = Hxz * Hyz - Hxy * Hzz;
    const double A02 = Hxy * Hyz - Hxz * Hyy;
    const double A12 = Hxy * Hxz - Hxx * Hyz;
    const double Ag0 = sum3(A00 * g0, A01 * g1, A02 * g2, leftAssoc);
    const double Ag1 = sum3(A01 * g0, A11 * g1, A12 * g2, leftAssoc);
    const double Ag2 = sum3(A02 * g0, A12 * g1, A22 * g2, leftAssoc);
    const double k = sum3(g0 * Ag0, g1 * Ag1, g2 * Ag2, leftAssoc);
    curv[1] = k / (z * z);
}

// One turn of ProjectToSurface's loop (include/hpsdf.h, "ProjectToSurface") after (f, g) = QueryGradient(x) with the world gradient:
// the stopping tests in their stated order, then the Newton step along g.  Returns the HPSDF_PROJECT_* status the point stops with, or
// -1 after x has moved (the caller counts the step).  One set of statements for the calling thread (host_query.cpp) and the kernels
// (project.hip).
__host__ __device__ inline int projectStep(double f, const double (&g)[3], double iso, double tol, uint32_t k, uint32_t maxIter,
                                           int leftAssoc, double (&x)[3]) {
    if (f == DBL_MAX) return 2;  // HPSDF_PROJECT_LEFT_ROOT
    const double r = f - iso;
    if (fabs(r) <= tol) return 0;  // HPSDF_PROJECT_CONVERGED
    const double z = sum3(g[0] * g[0], g[1] * g[1], g[2] * g[2], leftAssoc);
    if (!(z > 0.0)) return 3;    // HPSDF_PROJECT_FLAT
    if (k == maxIter) return 1;  // HPSDF_PROJECT_ITER_LIMIT
    const double s = r / z;
    x[0] = x[0] - s * g[0];
    x[1] = x[1] - s * g[1];
    x[2] = x[2] - s * g[2];
    return -1;
}

}  // namespace hpsdf

#if defined(__HIP__)
#include "leaf_eval.hpp"

namespace hpsdf {

struct DeviceBasisAt {
    __device__ int operator()(int r, int k) const { return kBasis.v[r][k]; }
};

// NPAIRS double2 loads into registers: a leaf's coefficients are 16-byte aligned in the device mirror and padded to an even count
// (hpsdf_tree_upload; evalLeafFixed reads them the same way)
template <int NPAIRS, int NV>
__device__ __forceinline__ void loadCoeffPairs(const double* __restrict__ c, double (&cv)[NV]) {
    static_assert(NV >= 2 * NPAIRS, "coefficient registers");
    const double2* __restrict__ c2 = reinterpret_cast<const double2*>(c);
#pragma unroll
    for (int i = 0; i < NPAIRS; ++i) {
        const double2 v = c2[i];
        cv[2 * i] = v.x;
        cv[2 * i + 1] = v.y;
    }
}

// leafJet for a compile-time degree with the leaf's coefficients in registers (cv)
template <int ORDER, int P, int NV>
__device__ __forceinline__ double leafJetVals(const double (&cv)[NV], const double (&u)[3], int depth, const double* sNl, const double* sRec,
                                              GradOut<ORDER> gu, HessOut<ORDER> hu) {
    static_assert(NV >= coeffCount(P), "coefficient registers");
    return leafJet<ORDER>(cv, FixedDegree<P>{}, coeffCount(P), u, depth, sNl, sRec, DeviceBasisAt{}, gu, hu);
}

// the leaf's coefficients from the device mirror, then the above
template <int ORDER, int P>
__device__ __forceinline__ double leafJetFixed(const double* __restrict__ c, const double (&u)[3], int depth, const double* sNl,
                                               const double* sRec, GradOut<ORDER> gu, HessOut<ORDER> hu) {
    constexpr int N = coeffCount(P);
    double cv[N + 1];
    loadCoeffPairs<(N + 1) / 2>(c, cv);
    return leafJetVals<ORDER, P>(cv, u, depth, sNl, sRec, gu, hu);
}

// any degree, tables in private memory: not inlined, like evalLeafGeneric
template <int ORDER>
__device__ __noinline__ double leafJetGeneric(const double* __restrict__ c, int degree, const double (&u)[3], int depth, const double* sNl,
                                              const double* sRec, GradOut<ORDER> gu, HessOut<ORDER> hu) {
    return leafJet<ORDER>(c, AnyDegree{degree}, coeffCount(degree), u, depth, sNl, sRec, DeviceBasisAt{}, gu, hu);
}

// the degree classes of evalLeaf<MAXP>: 2, 3 and 5 unrolled, 12 adds the any-degree code
template <int ORDER, int MAXP>
__device__ __forceinline__ double leafJetOf(const double* __restrict__ c, int degree, const double (&u)[3], int depth, const double* sNl,
                                            const double* sRec, GradOut<ORDER> gu, HessOut<ORDER> hu) {
    if (degree == 2) return leafJetFixed<ORDER, 2>(c, u, depth, sNl, sRec, gu, hu);
    if (degree == 1) return leafJetFixed<ORDER, 1>(c, u, depth, sNl, sRec, gu, hu);
    if (degree == 0) return leafJetFixed<ORDER, 0>(c, u, depth, sNl, sRec, gu, hu);
    if constexpr (MAXP >= 3) {
        if (degree == 3) return leafJetFixed<ORDER, 3>(c, u, depth, sNl, sRec, gu, hu);
    }
    if constexpr (MAXP >= 5) {
        if (degree == 4) return leafJetFixed<ORDER, 4>(c, u, depth, sNl, sRec, gu, hu);
        if (degree == 5) return leafJetFixed<ORDER, 5>(c, u, depth, sNl, sRec, gu, hu);
    }
    if constexpr (MAXP > 5) return leafJetGeneric<ORDER>(c, degree, u, depth, sNl, sRec, gu, hu);
    if constexpr (ORDER >= 1) gu[0] = gu[1] = gu[2] = 0.0;
    if constexpr (ORDER >= 2) hu[0] = hu[1] = hu[2] = hu[3] = hu[4] = hu[5] = 0.0;
    return 0.0;
}

}  // namespace hpsdf
#endif
