// A leaf's polynomial at a point and the per-point descent to it: evalLeaf*, queryPoint<MAXP>, and the staging of the
// normalisation / recurrence tables in LDS.  Included by kernels.hip (Query), by the fit units through field_glue.hpp (the
// CSG wrapper queries the old tree) and by fit.hip (fit_weight_kernel); depends on field_eval.hpp (sum3).
// evalLeafGeneric is not inlined and `static`: every code object that calls it carries its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_types.hpp"
#include "field_eval.hpp"

namespace hpsdf {

// ---------------------------------------------------------------------------
// tree evaluation: Octree::Query (Octree.cpp:662-702) and FApprox (:859-901)
// ---------------------------------------------------------------------------

// Basis index table in graded order (total degree, then first and second index).
struct BasisIdx {
    unsigned char v[456][3];
    constexpr BasisIdx() : v() {
        int row = 0;
        for (int p = 0; p <= 12; ++p)
            for (int a = 0; a <= p; ++a)
                for (int b = 0; a + b <= p; ++b) {
                    v[row][0] = (unsigned char)a;
                    v[row][1] = (unsigned char)b;
                    v[row][2] = (unsigned char)(p - a - b);
                    ++row;
                }
    }
};
__device__ constexpr BasisIdx kBasis{};
__host__ __device__ constexpr int coeffCount(int p) {
    // the reference's (u32)(1/6.0 * (p+1)*(p+2)*(p+3)) evaluates to 83 for p = 6
    return p == 6 ? 83 : (p + 1) * (p + 2) * (p + 3) / 6;
}

// sNl: [13][11] normalisation table, sRec: [13][2] recurrence constants (LDS).  cv holds the leaf's
// coefficients; values and summation order are those of Octree.cpp:888-898.
template <int P, int NV>
__device__ __forceinline__ double evalLeafVals(const double (&cv)[NV], double ux, double uy, double uz, int depth,
                                               const double* sNl, const double* sRec) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    double tx[P + 1], ty[P + 1], tz[P + 1];
    tx[0] = ty[0] = tz[0] = sNl[depth];
    double xm2 = 0.0, xm1 = 1.0, ym2 = 0.0, ym1 = 1.0, zm2 = 0.0, zm1 = 1.0;
#pragma unroll
    for (int j = 1; j <= P; ++j) {
        const double r0 = sRec[2 * j], r1 = sRec[2 * j + 1], nl = sNl[j * 11 + depth];
        const double lx = r0 * ux * xm1 - r1 * xm2;
        const double ly = r0 * uy * ym1 - r1 * ym2;
        const double lz = r0 * uz * zm1 - r1 * zm2;
        xm2 = xm1, xm1 = lx, ym2 = ym1, ym1 = ly, zm2 = zm1, zm1 = lz;
        tx[j] = lx * nl, ty[j] = ly * nl, tz[j] = lz * nl;
    }
    double f = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double lp = tx[kBasis.v[i][0]];
        lp = lp * ty[kBasis.v[i][1]];
        lp = lp * tz[kBasis.v[i][2]];
        f = f + cv[i] * lp;
    }
    return f;
}

// FApprox for the lanes of a wave whose leaves have different degrees <= P, in ONE pass: the basis rows of degree d are the first
// coeffCount(d) rows of the degree-P basis (Utility.h's table is ordered by total degree) and the sum runs row by row, so the value of
// a leaf of degree d is the running sum after row coeffCount(d) - 1 -- the very additions evalLeafVals<d> performs, on the same
// Legendre values (the recurrence is the same for j <= d) -- and each lane keeps the running sum at its own degree's last row.  A wave
// with degree-2 and degree-3 leaves used to run both bodies one after the other (tools/query_general_floor.py: the polynomial is a
// fifth of query_general's time); rows beyond a lane's degree multiply whatever its registers hold there: never read.
template <int P, int NV>
__device__ __forceinline__ double evalLeafValsMixed(const double (&cv)[NV], double ux, double uy, double uz, int depth, uint32_t degree,
                                                    const double* sNl, const double* sRec) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    double tx[P + 1], ty[P + 1], tz[P + 1];
    tx[0] = ty[0] = tz[0] = sNl[depth];
    double xm2 = 0.0, xm1 = 1.0, ym2 = 0.0, ym1 = 1.0, zm2 = 0.0, zm1 = 1.0;
#pragma unroll
    for (int j = 1; j <= P; ++j) {
        const double r0 = sRec[2 * j], r1 = sRec[2 * j + 1], nl = sNl[j * 11 + depth];
        const double lx = r0 * ux * xm1 - r1 * xm2;
        const double ly = r0 * uy * ym1 - r1 * ym2;
        const double lz = r0 * uz * zm1 - r1 * zm2;
        xm2 = xm1, xm1 = lx, ym2 = ym1, ym1 = ly, zm2 = zm1, zm1 = lz;
        tx[j] = lx * nl, ty[j] = ly * nl, tz[j] = lz * nl;
    }
    double f = 0.0, mine = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double lp = tx[kBasis.v[i][0]];
        lp = lp * ty[kBasis.v[i][1]];
        lp = lp * tz[kBasis.v[i][2]];
        f = f + cv[i] * lp;
#pragma unroll
        for (int dgr = 0; dgr < P; ++dgr)
            if (i == coeffCount(dgr) - 1) mine = degree == (uint32_t)dgr ? f : mine;
    }
    return degree == (uint32_t)P ? f : mine;
}

// Octree::FApproxWithGradient (Octree.cpp:904-985) for a compile-time degree: the value as FApprox, the "gradient"
// as the reference forms it -- per axis k the central difference of sum_r c_r * Lhat_{idx[r][k]}(u_k +- eps), i.e. with
// the other two axes' factors left out (:956-968) -- then normalised.  Same statements, same order as
// queryPointWithGradient's any-degree loop (and as the oracle), with the tables in registers.
template <int P, int NV>
__device__ __forceinline__ double evalLeafGradVals(const double (&cv)[NV], const double (&u)[3], int depth, const double* sNl,
                                                   const double* sRec, double (&g)[3], int left) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    const double eps = 0.0001;
    double L0[3][P + 1];  // normalised Legendre values at u, per axis: the value's factors
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double Lp[P + 1], Lm[P + 1];
        L0[k][0] = Lp[0] = Lm[0] = sNl[depth];
        double a2 = 0.0, a1 = 1.0, b2 = 0.0, b1 = 1.0, c2 = 0.0, c1 = 1.0;
#pragma unroll
        for (int j = 1; j <= P; ++j) {
            const double r0 = sRec[2 * j], r1 = sRec[2 * j + 1], nl = sNl[j * 11 + depth];
            const double a0 = r0 * u[k] * a1 - r1 * a2;          // :937
            const double b0 = r0 * (u[k] + eps) * b1 - r1 * b2;  // :941
            const double c0 = r0 * (u[k] - eps) * c1 - r1 * c2;  // :945
            a2 = a1, a1 = a0, b2 = b1, b1 = b0, c2 = c1, c1 = c0;
            L0[k][j] = a0 * nl, Lp[j] = b0 * nl, Lm[j] = c0 * nl;
        }
        double p1 = 0.0, m1 = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {  // :956-968
            p1 = p1 + cv[r] * Lp[kBasis.v[r][k]];
            m1 = m1 + cv[r] * Lm[kBasis.v[r][k]];
        }
        g[k] = (p1 - m1) / (2.0 * eps);
    }
    const double z = left ? sum3<true>(g[0] * g[0], g[1] * g[1], g[2] * g[2]) : sum3<false>(g[0] * g[0], g[1] * g[1], g[2] * g[2]);  // Eigen normalize()
    if (z > 0.0) {
        const double nrm = sqrt(z);
        g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
    }
    double f = 0.0;  // :972-984
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double lp = L0[0][kBasis.v[r][0]];
        lp = lp * L0[1][kBasis.v[r][1]];
        lp = lp * L0[2][kBasis.v[r][2]];
        f = f + cv[r] * lp;
    }
    return f;
}

// FApproxWithGradient for a wave's mix of degrees <= P in one pass, as evalLeafValsMixed: every running sum -- the two one-sided sums
// of each axis and the value -- is kept at the last row of the lane's own degree.
// (NODIV: lab builds only, tools/query_general_floor.py -- the six IEEE divisions and the square root left out)
template <int P, int NV, bool NODIV = false>
__device__ __forceinline__ double evalLeafGradValsMixed(const double (&cv)[NV], const double (&u)[3], int depth, uint32_t degree, const double* sNl,
                                                        const double* sRec, double (&g)[3], int left) {
    constexpr int N = coeffCount(P);
    static_assert(NV >= N, "coefficient registers");
    const double eps = 0.0001;
    double L0[3][P + 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double Lp[P + 1], Lm[P + 1];
        L0[k][0] = Lp[0] = Lm[0] = sNl[depth];
        double a2 = 0.0, a1 = 1.0, b2 = 0.0, b1 = 1.0, c2 = 0.0, c1 = 1.0;
#pragma unroll
        for (int j = 1; j <= P; ++j) {
            const double r0 = sRec[2 * j], r1 = sRec[2 * j + 1], nl = sNl[j * 11 + depth];
            const double a0 = r0 * u[k] * a1 - r1 * a2;          // :937
            const double b0 = r0 * (u[k] + eps) * b1 - r1 * b2;  // :941
            const double c0 = r0 * (u[k] - eps) * c1 - r1 * c2;  // :945
            a2 = a1, a1 = a0, b2 = b1, b1 = b0, c2 = c1, c1 = c0;
            L0[k][j] = a0 * nl, Lp[j] = b0 * nl, Lm[j] = c0 * nl;
        }
        double p1 = 0.0, m1 = 0.0, pMine = 0.0, mMine = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {  // :956-968
            p1 = p1 + cv[r] * Lp[kBasis.v[r][k]];
            m1 = m1 + cv[r] * Lm[kBasis.v[r][k]];
#pragma unroll
            for (int dgr = 0; dgr < P; ++dgr)
                if (r == coeffCount(dgr) - 1) pMine = degree == (uint32_t)dgr ? p1 : pMine, mMine = degree == (uint32_t)dgr ? m1 : mMine;
        }
        if (degree != (uint32_t)P) p1 = pMine, m1 = mMine;
        if constexpr (NODIV)
            g[k] = p1 - m1;
        else
            g[k] = (p1 - m1) / (2.0 * eps);
    }
    if constexpr (!NODIV) {
        const double z = left ? sum3<true>(g[0] * g[0], g[1] * g[1], g[2] * g[2]) : sum3<false>(g[0] * g[0], g[1] * g[1], g[2] * g[2]);  // Eigen normalize()
        if (z > 0.0) {
            const double nrm = sqrt(z);
            g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
        }
    }
    double f = 0.0, mine = 0.0;  // :972-984
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double lp = L0[0][kBasis.v[r][0]];
        lp = lp * L0[1][kBasis.v[r][1]];
        lp = lp * L0[2][kBasis.v[r][2]];
        f = f + cv[r] * lp;
#pragma unroll
        for (int dgr = 0; dgr < P; ++dgr)
            if (r == coeffCount(dgr) - 1) mine = degree == (uint32_t)dgr ? f : mine;
    }
    return degree == (uint32_t)P ? f : mine;
}

// Legendre recurrence constants (2j-1)/j and (j-1)/j (Include/HP/Utility.h:112-127): IEEE divisions of small
// integers, so the compile-time values are the table's values.
__host__ __device__ constexpr double recA(int j) { return j == 0 ? 0.0 : (2.0 * j - 1.0) / j; }
__host__ __device__ constexpr double recB(int j) { return j == 0 ? 0.0 : (j - 1.0) / j; }

// Same evaluation for a leaf sitting at the top-table level: its depth is uniform, so the normalisation
// factors arrive as kernel arguments (scalars) and the recurrence constants are literals.
template <int P, int NV>
__device__ __forceinline__ double evalLeafTop(const double (&cv)[NV], double ux, double uy, double uz,
                                              const double* __restrict__ nl) {
    constexpr int N = coeffCount(P);
    double tx[P + 1], ty[P + 1], tz[P + 1];
    tx[0] = ty[0] = tz[0] = nl[0];
    double xm2 = 0.0, xm1 = 1.0, ym2 = 0.0, ym1 = 1.0, zm2 = 0.0, zm1 = 1.0;
#pragma unroll
    for (int j = 1; j <= P; ++j) {
        const double lx = recA(j) * ux * xm1 - recB(j) * xm2;
        const double ly = recA(j) * uy * ym1 - recB(j) * ym2;
        const double lz = recA(j) * uz * zm1 - recB(j) * zm2;
        xm2 = xm1, xm1 = lx, ym2 = ym1, ym1 = ly, zm2 = zm1, zm1 = lz;
        tx[j] = lx * nl[j], ty[j] = ly * nl[j], tz[j] = lz * nl[j];
    }
    double f = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double lp = tx[kBasis.v[i][0]];
        lp = lp * ty[kBasis.v[i][1]];
        lp = lp * tz[kBasis.v[i][2]];
        f = f + cv[i] * lp;
    }
    return f;
}

// c is 16-byte aligned in the device mirror (hpsdf_tree_upload pads every leaf to an even count), so
// the coefficients come in as double2.
template <int P>
__device__ __forceinline__ double evalLeafFixed(const double* __restrict__ c, double ux, double uy, double uz, int depth,
                                                const double* sNl, const double* sRec) {
    constexpr int N = coeffCount(P);
    double cv[N + 1];
    const double2* __restrict__ c2 = reinterpret_cast<const double2*>(c);
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) {
        const double2 v = c2[i];
        cv[2 * i] = v.x;
        cv[2 * i + 1] = v.y;
    }
    return evalLeafVals<P>(cv, ux, uy, uz, depth, sNl, sRec);
}

// any degree (tables in private memory, dynamically indexed)
inline __device__ __noinline__ double evalLeafGeneric(const double* __restrict__ c, int degree, double ux, double uy, double uz,
                                               int depth, const double* sNl, const double* sRec) {
    double t[3][13];
    const double u[3] = {ux, uy, uz};
    for (int a = 0; a < 3; ++a) {
        t[a][0] = sNl[depth];
        double m2 = 0.0, m1 = 1.0;
        for (int j = 1; j <= degree; ++j) {
            const double l = sRec[2 * j] * u[a] * m1 - sRec[2 * j + 1] * m2;
            m2 = m1, m1 = l;
            t[a][j] = l * sNl[j * 11 + depth];
        }
    }
    double f = 0.0;
    const int n = coeffCount(degree);
    for (int i = 0; i < n; ++i) {
        double lp = t[0][kBasis.v[i][0]];
        lp = lp * t[1][kBasis.v[i][1]];
        lp = lp * t[2][kBasis.v[i][2]];
        f = f + c[i] * lp;
    }
    return f;
}

// MAXP: the largest leaf degree of the tree this instantiation serves (2, 3, 5 unrolled; 12 adds the
// generic path).  A smaller MAXP keeps registers (and so latency-hiding waves) for the common trees.
template <int MAXP>
__device__ __forceinline__ double evalLeaf(const double* __restrict__ c, int degree, double ux, double uy, double uz,
                                           int depth, const double* sNl, const double* sRec) {
    if constexpr (MAXP <= 2) {
        if (degree == 2) return evalLeafFixed<2>(c, ux, uy, uz, depth, sNl, sRec);
        if (degree == 1) return evalLeafFixed<1>(c, ux, uy, uz, depth, sNl, sRec);
        return evalLeafFixed<0>(c, ux, uy, uz, depth, sNl, sRec);
    } else {
        switch (degree) {
            case 0: return evalLeafFixed<0>(c, ux, uy, uz, depth, sNl, sRec);
            case 1: return evalLeafFixed<1>(c, ux, uy, uz, depth, sNl, sRec);
            case 2: return evalLeafFixed<2>(c, ux, uy, uz, depth, sNl, sRec);
            case 3: return evalLeafFixed<3>(c, ux, uy, uz, depth, sNl, sRec);
            default:
                if constexpr (MAXP >= 5) {
                    if (degree == 4) return evalLeafFixed<4>(c, ux, uy, uz, depth, sNl, sRec);
                    if (degree == 5) return evalLeafFixed<5>(c, ux, uy, uz, depth, sNl, sRec);
                }
                if constexpr (MAXP > 5) return evalLeafGeneric(c, degree, ux, uy, uz, depth, sNl, sRec);
                return 0.0;
        }
    }
}

// One point through the tree.  (x,y,z) in world coordinates.
template <int MAXP>
__device__ __forceinline__ double queryPoint(const TreeDev& t, double x, double y, double z, const double* sNl,
                                             const double* sRec) {
    // Octree.cpp:665
    const double px = (x - t.rootCentre[0]) * t.rootInvSizes[0];
    const double py = (y - t.rootCentre[1]) * t.rootInvSizes[1];
    const double pz = (z - t.rootCentre[2]) * t.rootInvSizes[2];
    // :668 containment on the f32 cast, both ends inclusive; NaN fails
    const float fx = (float)px, fy = (float)py, fz = (float)pz;
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) return DBL_MAX;
    // :674-701.  The mid-plane of a cell is its centre; centres are exact dyadics.  The levels that are
    // complete in this tree (topDepth of them; Octree::UniformlyRefine makes that 4) need no node reads:
    // the same comparisons give the path, and one table lookup gives the node reached.
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
    const uint32_t code = ix + ((iy + (iz << t.topDepth)) << t.topDepth);  // the table is indexed by cell (x, y, z)
    // One 128-byte line per top-level cell: the node record and, for a leaf of degree <= 2, its
    // coefficients inline -- the common case costs a single L2 line per point.  The coefficient loads
    // do not wait for the record (same line, issued together).
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
    if (rec.b <= 2u) {  // leaf at the table level, coefficients already here
        const double s = (double)(2 << depth);
        const double ux = (px - cx) * s, uy = (py - cy) * s, uz = (pz - cz) * s;
        if (rec.b == 2u) return evalLeafVals<2>(cv, ux, uy, uz, depth, sNl, sRec);
        if (rec.b == 1u) return evalLeafVals<1>(cv, ux, uy, uz, depth, sNl, sRec);
        return evalLeafVals<0>(cv, ux, uy, uz, depth, sNl, sRec);
    }
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
    // :862  unitPt = (pt - centre) * (2 << depth)
    const double s = (double)(2 << depth);
    return evalLeaf<MAXP>(t.coeffs + rec.a, (int)rec.b, (px - cx) * s, (py - cy) * s, (pz - cz) * s, depth, sNl, sRec);
}

__device__ __forceinline__ void stageQueryTables(const DeviceTables* T, double* sNl, double* sRec) {
    for (int i = threadIdx.x; i < 13 * 11; i += blockDim.x) sNl[i] = (&T->nl[0][0])[i];
    for (int i = threadIdx.x; i < 26; i += blockDim.x) sRec[i] = (&T->rec[0][0])[i];
}

// Cell of the complete top level that holds p (unit-cube coordinates), per axis: index k and cell centre c.
// The comparison chain "p >= mid-plane" of Octree.cpp:674-701, level by level, selects the cell k with
// lo_k <= p < lo_k + h (h = 2^-topDepth, lo_k = -0.5 + k h, all exact dyadics; k clamped to the grid because the
// containment test ran on the f32 cast).  k is computed directly -- floor((p+0.5)/h) can be off by one when
// p + 0.5 rounds across a cell boundary, so it is corrected by the same exact comparisons the chain would make.
__device__ __forceinline__ void topCell(const double (&p3)[3], int topDepth, int (&k3)[3], double (&c3)[3]) {
    const int side = 1 << topDepth;
    const double h = 1.0 / (double)side, fside = (double)side;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int k = (int)floor((p3[a] + 0.5) * fside);
        k = k < 0 ? 0 : (k > side - 1 ? side - 1 : k);
        double lo = -0.5 + (double)k * h;
        if (p3[a] < lo && k > 0) {
            --k;
            lo = lo - h;
        } else if (p3[a] >= lo + h && k < side - 1) {
            ++k;
            lo = lo + h;
        }
        k3[a] = k;
        c3[a] = lo + 0.5 * h;
    }
}

}  // namespace hpsdf
