// The gradient of a leaf's polynomial -- the derivative of what Query evaluates, not the reference's shortcut
// (FApproxWithGradient, Octree.cpp:904-985, kept as it is in leaf_eval.hpp's evalLeafGradVals) -- as include/hpsdf.h states it under
// "QueryGradient":
//   L_j(u_a)   Query's recurrence (Octree.cpp:876-885), D_0 = 0, D_1 = 1, D_j = D_{j-2} + (2j-1) L_{j-1};
//   LN_j = L_j nl[j][d], DN_j = D_j nl[j][d];
//   f          Query's running sum; gu_0 += c_r ((DN_a(x) LN_b(y)) LN_c(z)), gu_1 += c_r ((LN_a DN_b) LN_c), gu_2 += c_r ((LN_a LN_b) DN_c);
//   g_a = (gu_a (double)(2 << d)) rootInvSizes[a]; HPSDF_GRADIENT_UNIT: z = sum3(g^2) in the context's order, g_a / sqrt(z) if z > 0.
// One set of statements for the calling thread (host_query.cpp: leafTrueGradient, the first half of this file, plain C++) and for the
// kernels (query_gradient.hip: the second half, the same statements with the degree at compile time and the tables in registers).
// Everything is built with -ffp-contract=off, so both give the same bits.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace hpsdf {

// Any degree.  co: the leaf's coefficients in basis order; nl: [13][11] normalisation table, rec: [13][2] recurrence constants (flat);
// bidx(r, k): index k of basis row r.  Returns f, leaves the unit-space partials in gu.
template <class BasisAt>
__host__ __device__ inline double leafTrueGradient(const double* co, int degree, int nc, const double (&u)[3], int depth, const double* nl,
                                                   const double* rec, BasisAt bidx, double (&gu)[3]) {
    double LN[3][13], DN[3][13];
    for (int a = 0; a < 3; ++a) {
        LN[a][0] = nl[depth];
        DN[a][0] = 0.0 * nl[depth];
        double m2 = 0.0, m1 = 1.0, d2 = 0.0, d1 = 0.0;  // L_{j-2}, L_{j-1}, D_{j-2}, D_{j-1}
        for (int j = 1; j <= degree; ++j) {
            const double n = nl[j * 11 + depth];
            const double l = rec[2 * j] * u[a] * m1 - rec[2 * j + 1] * m2;
            const double d = j == 1 ? 1.0 : d2 + (double)(2 * j - 1) * m1;
            m2 = m1, m1 = l, d2 = d1, d1 = d;
            LN[a][j] = l * n;
            DN[a][j] = d * n;
        }
    }
    double f = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int r = 0; r < nc; ++r) {
        const int a = bidx(r, 0), b = bidx(r, 1), c = bidx(r, 2);
        double lp = LN[0][a];
        lp = lp * LN[1][b];
        lp = lp * LN[2][c];
        f = f + co[r] * lp;
        g0 = g0 + co[r] * ((DN[0][a] * LN[1][b]) * LN[2][c]);
        g1 = g1 + co[r] * ((LN[0][a] * DN[1][b]) * LN[2][c]);
        g2 = g2 + co[r] * ((LN[0][a] * LN[1][b]) * DN[2][c]);
    }
    gu[0] = g0, gu[1] = g1, gu[2] = g2;
    return f;
}

// unit-space partials -> world gradient (the chain rule through Octree.cpp:862 and :665), normalised under HPSDF_GRADIENT_UNIT
__host__ __device__ inline void finishTrueGradient(const double (&gu)[3], int depth, const double* rootInvSizes, bool unit, int leftAssoc,
                                                   double (&g)[3]) {
    const double s = (double)(2 << depth);
    g[0] = (gu[0] * s) * rootInvSizes[0];
    g[1] = (gu[1] * s) * rootInvSizes[1];
    g[2] = (gu[2] * s) * rootInvSizes[2];
    if (unit) {
        const double a = g[0] * g[0], b = g[1] * g[1], c = g[2] * g[2];
        const double z = leftAssoc ? (a + b) + c : a + (b + c);
        if (z > 0.0) {
            const double nrm = sqrt(z);
            g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
        }
    }
}

// finishTrueGradient's normalisation on its own, for a world gradient that already went through it with unit = false
__host__ __device__ inline void unitGradient(double (&g)[3], int leftAssoc) {
    const double a = g[0] * g[0], b = g[1] * g[1], c = g[2] * g[2];
    const double z = leftAssoc ? (a + b) + c : a + (b + c);
    if (z > 0.0) {
        const double nrm = sqrt(z);
        g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
    }
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
    const double a = g[0] * g[0], b = g[1] * g[1], c = g[2] * g[2];
    const double z = leftAssoc ? (a + b) + c : a + (b + c);
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

// leafTrueGradient for a compile-time degree, the leaf's coefficients in registers (cv) and every table entry a register: the
// statements above, unrolled.
template <int P, int NV>
__device__ __forceinline__ double leafTrueGradientVals(const double (&cv)[NV], const double (&u)[3], int depth, const double* sNl,
                                                       const double* sRec, double (&gu)[3]) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    double LN[3][P + 1], DN[3][P + 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        LN[a][0] = sNl[depth];
        DN[a][0] = 0.0 * sNl[depth];
        double m2 = 0.0, m1 = 1.0, d2 = 0.0, d1 = 0.0;
#pragma unroll
        for (int j = 1; j <= P; ++j) {
            const double n = sNl[j * 11 + depth];
            const double l = sRec[2 * j] * u[a] * m1 - sRec[2 * j + 1] * m2;
            const double d = j == 1 ? 1.0 : d2 + (double)(2 * j - 1) * m1;
            m2 = m1, m1 = l, d2 = d1, d1 = d;
            LN[a][j] = l * n;
            DN[a][j] = d * n;
        }
    }
    double f = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        const int a = kBasis.v[r][0], b = kBasis.v[r][1], c = kBasis.v[r][2];
        double lp = LN[0][a];
        lp = lp * LN[1][b];
        lp = lp * LN[2][c];
        f = f + cv[r] * lp;
        g0 = g0 + cv[r] * ((DN[0][a] * LN[1][b]) * LN[2][c]);
        g1 = g1 + cv[r] * ((LN[0][a] * DN[1][b]) * LN[2][c]);
        g2 = g2 + cv[r] * ((LN[0][a] * LN[1][b]) * DN[2][c]);
    }
    gu[0] = g0, gu[1] = g1, gu[2] = g2;
    return f;
}

// the leaf's coefficients from the device mirror (16-byte aligned, padded to an even count: evalLeafFixed), then the above
template <int P>
__device__ __forceinline__ double leafTrueGradientFixed(const double* __restrict__ c, const double (&u)[3], int depth, const double* sNl,
                                                        const double* sRec, double (&gu)[3]) {
    constexpr int N = coeffCount(P);
    double cv[N + 1];
    const double2* __restrict__ c2 = reinterpret_cast<const double2*>(c);
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) {
        const double2 v = c2[i];
        cv[2 * i] = v.x;
        cv[2 * i + 1] = v.y;
    }
    return leafTrueGradientVals<P>(cv, u, depth, sNl, sRec, gu);
}

struct DeviceBasisAt {
    __device__ int operator()(int r, int k) const { return kBasis.v[r][k]; }
};

// any degree, tables in private memory: not inlined, like evalLeafGeneric
inline __device__ __noinline__ double leafTrueGradientGeneric(const double* __restrict__ c, int degree, const double (&u)[3], int depth,
                                                              const double* sNl, const double* sRec, double (&gu)[3]) {
    return leafTrueGradient(c, degree, coeffCount(degree), u, depth, sNl, sRec, DeviceBasisAt{}, gu);
}

// the degree classes of evalLeaf<MAXP>: 2, 3 and 5 unrolled, 12 adds the any-degree code
template <int MAXP>
__device__ __forceinline__ double leafTrueGradientOf(const double* __restrict__ c, int degree, const double (&u)[3], int depth,
                                                     const double* sNl, const double* sRec, double (&gu)[3]) {
    if (degree == 2) return leafTrueGradientFixed<2>(c, u, depth, sNl, sRec, gu);
    if (degree == 1) return leafTrueGradientFixed<1>(c, u, depth, sNl, sRec, gu);
    if (degree == 0) return leafTrueGradientFixed<0>(c, u, depth, sNl, sRec, gu);
    if constexpr (MAXP >= 3) {
        if (degree == 3) return leafTrueGradientFixed<3>(c, u, depth, sNl, sRec, gu);
    }
    if constexpr (MAXP >= 5) {
        if (degree == 4) return leafTrueGradientFixed<4>(c, u, depth, sNl, sRec, gu);
        if (degree == 5) return leafTrueGradientFixed<5>(c, u, depth, sNl, sRec, gu);
    }
    if constexpr (MAXP > 5) return leafTrueGradientGeneric(c, degree, u, depth, sNl, sRec, gu);
    gu[0] = gu[1] = gu[2] = 0.0;
    return 0.0;
}

}  // namespace hpsdf
#endif
