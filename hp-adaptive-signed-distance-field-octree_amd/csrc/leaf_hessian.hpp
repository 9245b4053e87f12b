// The second derivative of a leaf's polynomial and the curvature of its level set, as include/hpsdf.h states them under "QueryHessian":
//   L_j, D_j, LN_j, DN_j   QueryGradient's (leaf_gradient.hpp);  E_0 = E_1 = 0, E_j = E_{j-2} + (2j-1) D_{j-1} (= L_j'');  EN_j = E_j nl[j][d];
//   f, gu_0..2             QueryGradient's statements in their order (the same bits);
//   hu_xx += c_r ((EN_a LN_b) LN_c), hu_yy += c_r ((LN_a EN_b) LN_c), hu_zz += c_r ((LN_a LN_b) EN_c),
//   hu_xy += c_r ((DN_a DN_b) LN_c), hu_xz += c_r ((DN_a LN_b) DN_c), hu_yz += c_r ((LN_a DN_b) DN_c);
//   H_ab = (((hu_ab s) s) rootInvSizes[a]) rootInvSizes[b], s = (double)(2 << d); stored xx, yy, zz, xy, xz, yz;
//   curv = (mean, gauss) of the level set through the point, from the un-normalised world gradient and H.
// One set of statements for the calling thread (host_query.cpp: leafHessian, the first half of this file, plain C++) and for the
// kernels (query_hessian.hip: the second half, the same statements with the degree at compile time and the tables in registers).
// Everything is built with -ffp-contract=off, so both give the same bits.
#pragma once
#include "leaf_gradient.hpp"

namespace hpsdf {

// Any degree; the arguments of leafTrueGradient.  Returns f, leaves the unit-space first partials in gu and the second in hu.
template <class BasisAt>
__host__ __device__ inline double leafHessian(const double* co, int degree, int nc, const double (&u)[3], int depth, const double* nl,
                                              const double* rec, BasisAt bidx, double (&gu)[3], double (&hu)[6]) {
    double LN[3][13], DN[3][13], EN[3][13];
    for (int a = 0; a < 3; ++a) {
        LN[a][0] = nl[depth];
        DN[a][0] = 0.0 * nl[depth];
        EN[a][0] = 0.0 * nl[depth];
        double m2 = 0.0, m1 = 1.0, d2 = 0.0, d1 = 0.0, e2 = 0.0, e1 = 0.0;  // L, D, E of j-2 and j-1
        for (int j = 1; j <= degree; ++j) {
            const double n = nl[j * 11 + depth];
            const double l = rec[2 * j] * u[a] * m1 - rec[2 * j + 1] * m2;
            const double d = j == 1 ? 1.0 : d2 + (double)(2 * j - 1) * m1;
            const double e = j == 1 ? 0.0 : e2 + (double)(2 * j - 1) * d1;
            m2 = m1, m1 = l, d2 = d1, d1 = d, e2 = e1, e1 = e;
            LN[a][j] = l * n;
            DN[a][j] = d * n;
            EN[a][j] = e * n;
        }
    }
    double f = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, hxx = 0.0, hyy = 0.0, hzz = 0.0, hxy = 0.0, hxz = 0.0, hyz = 0.0;
    for (int r = 0; r < nc; ++r) {
        const int a = bidx(r, 0), b = bidx(r, 1), c = bidx(r, 2);
        double lp = LN[0][a];
        lp = lp * LN[1][b];
        lp = lp * LN[2][c];
        f = f + co[r] * lp;
        g0 = g0 + co[r] * ((DN[0][a] * LN[1][b]) * LN[2][c]);
        g1 = g1 + co[r] * ((LN[0][a] * DN[1][b]) * LN[2][c]);
        g2 = g2 + co[r] * ((LN[0][a] * LN[1][b]) * DN[2][c]);
        hxx = hxx + co[r] * ((EN[0][a] * LN[1][b]) * LN[2][c]);
        hyy = hyy + co[r] * ((LN[0][a] * EN[1][b]) * LN[2][c]);
        hzz = hzz + co[r] * ((LN[0][a] * LN[1][b]) * EN[2][c]);
        hxy = hxy + co[r] * ((DN[0][a] * DN[1][b]) * LN[2][c]);
        hxz = hxz + co[r] * ((DN[0][a] * LN[1][b]) * DN[2][c]);
        hyz = hyz + co[r] * ((LN[0][a] * DN[1][b]) * DN[2][c]);
    }
    gu[0] = g0, gu[1] = g1, gu[2] = g2;
    hu[0] = hxx, hu[1] = hyy, hu[2] = hzz, hu[3] = hxy, hu[4] = hxz, hu[5] = hyz;
    return f;
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

__host__ __device__ inline double hessianSum3(double a, double b, double c, int leftAssoc) { return leftAssoc ? (a + b) + c : a + (b + c); }

// Mean and Gaussian curvature of the level set through the point, from the world gradient (NOT normalised) and the world Hessian:
// mean = (|g|^2 tr H - g.Hg) / (2 |g|^3), gauss = g.adj(H)g / |g|^4; a field positive outside gives a sphere of radius r (1/r, 1/r^2).
// A zero (or NaN) gradient: two quiet NaNs.
__host__ __device__ inline void levelSetCurvature(const double (&g)[3], const double (&H)[6], int leftAssoc, double (&curv)[2]) {
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    const double Hxx = H[0], Hyy = H[1], Hzz = H[2], Hxy = H[3], Hxz = H[4], Hyz = H[5];
    const double z = hessianSum3(g0 * g0, g1 * g1, g2 * g2, leftAssoc);
    if (!(z > 0.0)) {
        curv[0] = curv[1] = __builtin_nan("");
        return;
    }
    const double Hg0 = hessianSum3(Hxx * g0, Hxy * g1, Hxz * g2, leftAssoc);
    const double Hg1 = hessianSum3(Hxy * g0, Hyy * g1, Hyz * g2, leftAssoc);
    const double Hg2 = hessianSum3(Hxz * g0, Hyz * g1, Hzz * g2, leftAssoc);
    const double q = hessianSum3(g0 * Hg0, g1 * Hg1, g2 * Hg2, leftAssoc);
    const double tr = hessianSum3(Hxx, Hyy, Hzz, leftAssoc);
    curv[0] = (z * tr - q) / ((2.0 * z) * sqrt(z));
    const double A00 = Hyy * Hzz - Hyz * Hyz;
    const double A11 = Hxx * Hzz - Hxz * Hxz;
    const double A22 = Hxx * Hyy - Hxy * Hxy;
    const double A01 = Hxz * Hyz - Hxy * Hzz;
    const double A02 = Hxy * Hyz - Hxz * Hyy;
    const double A12 = Hxy * Hxz - Hxx * Hyz;
    const double Ag0 = hessianSum3(A00 * g0, A01 * g1, A02 * g2, leftAssoc);
    const double Ag1 = hessianSum3(A01 * g0, A11 * g1, A12 * g2, leftAssoc);
    const double Ag2 = hessianSum3(A02 * g0, A12 * g1, A22 * g2, leftAssoc);
    const double k = hessianSum3(g0 * Ag0, g1 * Ag1, g2 * Ag2, leftAssoc);
    curv[1] = k / (z * z);
}

}  // namespace hpsdf

#if defined(__HIP__)

namespace hpsdf {

// leafHessian for a compile-time degree, the leaf's coefficients in registers (cv) and every table entry a register: the statements
// above, unrolled.
template <int P, int NV>
__device__ __forceinline__ double leafHessianVals(const double (&cv)[NV], const double (&u)[3], int depth, const double* sNl,
                                                  const double* sRec, double (&gu)[3], double (&hu)[6]) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    double LN[3][P + 1], DN[3][P + 1], EN[3][P + 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        LN[a][0] = sNl[depth];
        DN[a][0] = 0.0 * sNl[depth];
        EN[a][0] = 0.0 * sNl[depth];
        double m2 = 0.0, m1 = 1.0, d2 = 0.0, d1 = 0.0, e2 = 0.0, e1 = 0.0;
#pragma unroll
        for (int j = 1; j <= P; ++j) {
            const double n = sNl[j * 11 + depth];
            const double l = sRec[2 * j] * u[a] * m1 - sRec[2 * j + 1] * m2;
            const double d = j == 1 ? 1.0 : d2 + (double)(2 * j - 1) * m1;
            const double e = j == 1 ? 0.0 : e2 + (double)(2 * j - 1) * d1;
            m2 = m1, m1 = l, d2 = d1, d1 = d, e2 = e1, e1 = e;
            LN[a][j] = l * n;
            DN[a][j] = d * n;
            EN[a][j] = e * n;
        }
    }
    double f = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, hxx = 0.0, hyy = 0.0, hzz = 0.0, hxy = 0.0, hxz = 0.0, hyz = 0.0;
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
        hxx = hxx + cv[r] * ((EN[0][a] * LN[1][b]) * LN[2][c]);
        hyy = hyy + cv[r] * ((LN[0][a] * EN[1][b]) * LN[2][c]);
        hzz = hzz + cv[r] * ((LN[0][a] * LN[1][b]) * EN[2][c]);
        hxy = hxy + cv[r] * ((DN[0][a] * DN[1][b]) * LN[2][c]);
        hxz = hxz + cv[r] * ((DN[0][a] * LN[1][b]) * DN[2][c]);
        hyz = hyz + cv[r] * ((LN[0][a] * DN[1][b]) * DN[2][c]);
    }
    gu[0] = g0, gu[1] = g1, gu[2] = g2;
    hu[0] = hxx, hu[1] = hyy, hu[2] = hzz, hu[3] = hxy, hu[4] = hxz, hu[5] = hyz;
    return f;
}

// the leaf's coefficients from the device mirror (16-byte aligned, padded to an even count: evalLeafFixed), then the above
template <int P>
__device__ __forceinline__ double leafHessianFixed(const double* __restrict__ c, const double (&u)[3], int depth, const double* sNl,
                                                   const double* sRec, double (&gu)[3], double (&hu)[6]) {
    constexpr int N = coeffCount(P);
    double cv[N + 1];
    const double2* __restrict__ c2 = reinterpret_cast<const double2*>(c);
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) {
        const double2 v = c2[i];
        cv[2 * i] = v.x;
        cv[2 * i + 1] = v.y;
    }
    return leafHessianVals<P>(cv, u, depth, sNl, sRec, gu, hu);
}

// any degree, tables in private memory: not inlined, like leafTrueGradientGeneric
inline __device__ __noinline__ double leafHessianGeneric(const double* __restrict__ c, int degree, const double (&u)[3], int depth,
                                                         const double* sNl, const double* sRec, double (&gu)[3], double (&hu)[6]) {
    return leafHessian(c, degree, coeffCount(degree), u, depth, sNl, sRec, DeviceBasisAt{}, gu, hu);
}

// the degree classes of leafTrueGradientOf<MAXP>: 2, 3 and 5 unrolled, 12 adds the any-degree code
template <int MAXP>
__device__ __forceinline__ double leafHessianOf(const double* __restrict__ c, int degree, const double (&u)[3], int depth, const double* sNl,
                                                const double* sRec, double (&gu)[3], double (&hu)[6]) {
    if (degree == 2) return leafHessianFixed<2>(c, u, depth, sNl, sRec, gu, hu);
    if (degree == 1) return leafHessianFixed<1>(c, u, depth, sNl, sRec, gu, hu);
    if (degree == 0) return leafHessianFixed<0>(c, u, depth, sNl, sRec, gu, hu);
    if constexpr (MAXP >= 3) {
        if (degree == 3) return leafHessianFixed<3>(c, u, depth, sNl, sRec, gu, hu);
    }
    if constexpr (MAXP >= 5) {
        if (degree == 4) return leafHessianFixed<4>(c, u, depth, sNl, sRec, gu, hu);
        if (degree == 5) return leafHessianFixed<5>(c, u, depth, sNl, sRec, gu, hu);
    }
    if constexpr (MAXP > 5) return leafHessianGeneric(c, degree, u, depth, sNl, sRec, gu, hu);
    gu[0] = gu[1] = gu[2] = 0.0;
    hu[0] = hu[1] = hu[2] = hu[3] = hu[4] = hu[5] = 0.0;
    return 0.0;
}

}  // namespace hpsdf
#endif
