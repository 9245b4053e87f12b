// IntegratePair (include/hpsdf.h, "IntegratePair"): the plain C++ part -- the pose and the image box of a cell, the clamp to B's root, a
// cell's class against both trees and a final cell's row.  Integrate's cells, lists, reduction and world transform (integrate.hpp) are used
// as they are; B is bounded by QueryBounds' walk (tree_bound.hpp, boundsWalkRange) and sampled by Query's point descent.  Shared by
// integrate_pair.hip (the kernels) and integrate_pair_host.cpp (the same loop over host lists): one set of statements with a fixed
// association, built with -ffp-contract=off, so host and device give the same bits.  No HIP compiler is needed for this file.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "integrate.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

constexpr double kPairPMax = 0.5 + 1.0 / 33554432.0;  // 0.5 + 2^-25: the largest double whose (float) cast is <= 0.5f (ties to even)
constexpr double kPairPMin = -kPairPMax;
constexpr double kPairSlack = 32.0 / 9007199254740992.0;  // 32 * 2^-53 (include/hpsdf.h: 17 roundings counted, headroom 32 / 17)

// What a call's cells are classified with.  delta and sizeA are made once, on the host, by pairArgs: kernels and host loop read the same
// doubles.
struct PairArgs {
    double isoA, isoB;
    double M[9], t[3];  // y = M x + t, row-major
    double delta[3];    // the slack of row j of the image box
    double sizeA[3];    // 1.0 / rootInvSizes of A
    uint32_t op, maxLeaves;
};

// delta_j = kPairSlack * (((|M_j0| X_0 + |M_j1| X_1) + |M_j2| X_2) + |t_j|), X_k = |rootCentreA_k| + 0.5 * sizeA_k: the largest
// magnitudes any point of A's root brings into row j
inline PairArgs pairArgs(const ClsTree& tA, uint32_t op, const double* pose, double isoA, double isoB, uint32_t maxLeaves) {
    PairArgs a{};
    a.isoA = isoA, a.isoB = isoB, a.op = op, a.maxLeaves = maxLeaves;
    double X[3];
    for (int k = 0; k < 3; ++k) {
        a.sizeA[k] = 1.0 / tA.rootInvSizes[k];
        X[k] = std::fabs(tA.rootCentre[k]) + 0.5 * a.sizeA[k];
    }
    for (int j = 0; j < 3; ++j) {
        for (int k = 0; k < 3; ++k) a.M[3 * j + k] = pose[4 * j + k];
        a.t[j] = pose[4 * j + 3];
        const double* m = a.M + 3 * j;
        a.delta[j] = kPairSlack * (((std::fabs(m[0]) * X[0] + std::fabs(m[1]) * X[1]) + std::fabs(m[2]) * X[2]) + std::fabs(a.t[j]));
    }
    return a;
}

// what hpsdf_integrate_pair_* reject before anything runs (0: fine)
int pairArgumentError(uint32_t op, const double* pose, double isoA, double isoB, uint32_t depth, uint32_t samples, uint32_t maxCells,
                      uint32_t maxLeaves, const void* out, const void* outCells, const void* outCount);

// y = M x + t, the statement of the header's steps 3 and 6
__host__ __device__ inline void pairImage(const PairArgs& a, const double (&x)[3], double (&y)[3]) {
    for (int j = 0; j < 3; ++j) {
        const double* m = a.M + 3 * j;
        y[j] = ((m[0] * x[0] + m[1] * x[1]) + m[2] * x[2]) + a.t[j];
    }
}

// The centre cx and the half edges hx of cell c in A's world frame (step 3's first statements; Clearance's witness is cx, clearance.hpp)
__host__ __device__ inline void pairCellCentre(const ClsTree& tA, const PairArgs& a, const IntegrateCell& c, double (&cx)[3], double (&hx)[3]) {
    const double s = 1.0 / (double)(1u << c.depth);
    const double ijk[3] = {(double)c.i, (double)c.j, (double)c.k};
    for (int k = 0; k < 3; ++k) {
        const double pc = (-0.5 + ijk[k] * s) + 0.5 * s;  // exact
        cx[k] = tA.rootCentre[k] + pc * a.sizeA[k];
        hx[k] = (0.5 * s) * a.sizeA[k];
    }
}

// The image box [lo, hi] of cell c in B's world frame (step 3)
__host__ __device__ inline void pairCellBox(const ClsTree& tA, const PairArgs& a, const IntegrateCell& c, double (&lo)[3], double (&hi)[3]) {
    double cx[3], hx[3];
    pairCellCentre(tA, a, c, cx, hx);
    double yc[3];
    pairImage(a, cx, yc);
    for (int j = 0; j < 3; ++j) {
        const double* m = a.M + 3 * j;
        const double r = (fabs(m[0]) * hx[0] + fabs(m[1]) * hx[1]) + fabs(m[2]) * hx[2];
        const double rd = r + a.delta[j];
        lo[j] = yc[j] - rd;
        hi[j] = yc[j] + rd;
    }
}

// Step 4: the box in B's normalised frame, clamped to what passes Query's containment test.  0: walk [pl, ph]; 1: no point of the box
// reaches B; 3: a NaN, nothing is known.  *partial: part of the box lies outside B's root.
__host__ __device__ inline uint32_t pairClamp(const ClsTree& tB, const double (&lo)[3], const double (&hi)[3], double (&pl)[3], double (&ph)[3],
                                              bool* partial) {
    *partial = false;
    bool nan = false, miss = false;
    for (int k = 0; k < 3; ++k) {
        pl[k] = (lo[k] - tB.rootCentre[k]) * tB.rootInvSizes[k];
        ph[k] = (hi[k] - tB.rootCentre[k]) * tB.rootInvSizes[k];
        if (pl[k] != pl[k] || ph[k] != ph[k]) nan = true;
        if ((float)ph[k] < -0.5f || (float)pl[k] > 0.5f) miss = true;
        if (!((float)pl[k] >= -0.5f)) pl[k] = kPairPMin, *partial = true;
        if (!((float)ph[k] <= 0.5f)) ph[k] = kPairPMax, *partial = true;
    }
    return nan ? 3u : (miss ? 1u : 0u);
}

// The class of the cell's image against B (steps 3 to 5): 1 outside, 2 inside, 0 undecided.  *finite: false if the walk met a leaf
// that is not finite.
template <class Eval, class Stack>
__host__ __device__ inline uint32_t pairClassB(const ClsTree& tA, const ClsTree& tB, const PairArgs& a, const IntegrateCell& c, const Eval& eval,
                                               Stack& st, bool* finite) {
    double lo[3], hi[3], pl[3], ph[3];
    bool partial;
    pairCellBox(tA, a, c, lo, hi);
    const uint32_t reach = pairClamp(tB, lo, hi, pl, ph, &partial);
    if (reach != 0u) return reach == 1u ? 1u : 0u;
    BoundsRow R;
    boundsWalkRange(tB, pl, ph, 1u, a.maxLeaves, eval, st, R);
    if (R.status == HPSDF_BOUNDS_NOT_FINITE) *finite = false;
    if (R.lo > a.isoB) return 1u;
    if (R.hi < a.isoB && !partial) return 2u;
    return 0u;
}

// Step 6's table: the class of the operation from the two classes
__host__ __device__ inline uint32_t pairCombine(uint32_t op, uint32_t clsA, uint32_t clsB) {
    if (op == HPSDF_PAIR_INTERSECTION) return clsA == 1u || clsB == 1u ? 1u : (clsA == 2u && clsB == 2u ? 2u : 0u);
    if (op == HPSDF_PAIR_UNION) return clsA == 1u && clsB == 1u ? 1u : (clsA == 2u || clsB == 2u ? 2u : 0u);
    return clsA == 1u || clsB == 2u ? 1u : (clsA == 2u && clsB == 1u ? 2u : 0u);
}
__host__ __device__ inline bool pairPredicate(uint32_t op, bool inA, bool inB) {
    if (op == HPSDF_PAIR_INTERSECTION) return inA && inB;
    if (op == HPSDF_PAIR_UNION) return inA || inB;
    return inA && !inB;
}

// Class of a cell (include/hpsdf.h, "IntegratePair", "Class of a cell"): 1 outside, 2 inside, 0 undecided
template <class Eval, class Stack>
__host__ __device__ inline uint32_t pairCellClass(const ClsTree& tA, const ClsTree& tB, const PairArgs& a, const IntegrateCell& c, int level,
                                                  const Eval& eval, Stack& st, bool* finite) {
    const uint32_t clsA = integrateCellClass(tA, c, level, a.isoA, eval, finite);
    if (!*finite) return 0u;
    if (a.op == HPSDF_PAIR_UNION ? clsA == 2u : clsA == 1u) return clsA;  // A decides alone: B is not touched
    return pairCombine(a.op, clsA, pairClassB(tA, tB, a, c, eval, st, finite));
}

// Query_B(y) by Query's point descent (leaf_eval.hpp, queryPoint; host_query.cpp, descend): the root map, the containment test on the f32
// cast, the mid-plane descent, the leaf's polynomial.  DBL_MAX outside B's root and for a NaN.
template <class Eval>
__host__ __device__ inline double pairQueryPoint(const ClsTree& t, const double (&y)[3], const Eval& eval) {
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = (y[k] - t.rootCentre[k]) * t.rootInvSizes[k];
    const float fx = (float)p[0], fy = (float)p[1], fz = (float)p[2];
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) return DBL_MAX;
    double cx = 0.0, cy = 0.0, cz = 0.0, q = 0.25;
    int depth = 0;
    NodeRec rec = t.nodes[0];
    while (rec.b == kInteriorTag && depth < kLevels) {
        const bool ux = p[0] >= cx, uy = p[1] >= cy, uz = p[2] >= cz;
        const uint32_t idx = rec.a + (ux ? 1u : 0u) + (uy ? 2u : 0u) + (uz ? 4u : 0u);
        cx = ux ? cx + q : cx - q;
        cy = uy ? cy + q : cy - q;
        cz = uz ? cz + q : cz - q;
        q = q * 0.5;
        ++depth;
        rec = t.nodes[idx];
    }
    const double s = (double)(2 << depth);
    return eval(t.coeffs + rec.a, (int)rec.b, (p[0] - cx) * s, (p[1] - cy) * s, (p[2] - cz) * s, depth);
}

// The row of a FINAL cell; c.cls holds its class.  integrateCellRow's statements, with the operation's predicate on (inA, inB) where
// Integrate has f < iso.
template <class Eval>
__host__ __device__ inline void pairCellRow(const ClsTree& tA, const ClsTree& tB, const PairArgs& a, const IntegrateCell& c, int level, uint32_t q,
                                            const Eval& eval, double (&row)[kIntRow]) {
    for (int k = 0; k < kIntRow; ++k) row[k] = 0.0;
    if (c.cls == 1u) {
        row[kIntCellsOut] = 1.0;
        return;
    }
    const double s = 1.0 / (double)(1u << c.depth);
    const double v = (s * s) * s;
    const double plo[3] = {-0.5 + (double)c.i * s, -0.5 + (double)c.j * s, -0.5 + (double)c.k * s};
    double m[10];
    if (c.cls == 2u) {
        const double cen[3] = {plo[0] + 0.5 * s, plo[1] + 0.5 * s, plo[2] + 0.5 * s};
        integrateBoxMoments(v, cen, s, m);
        for (int k = 0; k < 10; ++k) row[kIntM0 + k] = m[k];
        row[kIntLo] = v;
        row[kIntCellsIn] = 1.0;
        return;
    }
    row[kIntUnd] = v;
    row[kIntCellsUnd] = 1.0;
    double lo[3], w;
    integrateCellLo(c, level, lo, w);
    const uint32_t shift = q >> 1;  // log2(q) for 1, 2, 4
    const double part = 1.0 / (double)q;
    const double hu = (0.5 * w) * part;  // half a sub-box's edge in u
    const double ss = s * part;          // a sub-box's edge in p
    const double hs = 0.5 * ss;
    const double vs = (ss * ss) * ss;
    const NodeRec rec = tA.nodes[c.node];
    const uint32_t count = 1u << (3u * shift);
    for (uint32_t n = 0; n < count; ++n) {  // x fastest, then y, then z
        const uint32_t idx[3] = {n & (q - 1u), (n >> shift) & (q - 1u), n >> (2u * shift)};
        double u[3], p[3];
        for (int k = 0; k < 3; ++k) {
            const double odd = (double)(2u * idx[k] + 1u);
            u[k] = lo[k] + odd * hu;
            p[k] = plo[k] + odd * hs;
        }
        const double f = eval(tA.coeffs + rec.a, (int)rec.b, u[0], u[1], u[2], (int)c.depth - level);
        const bool inA = f < a.isoA;
        bool inB = false;
        if (a.op == HPSDF_PAIR_UNION ? !inA : inA) {  // (where inA decides the predicate alone, B is not asked)
            double x[3], y[3];
            for (int k = 0; k < 3; ++k) x[k] = tA.rootCentre[k] + p[k] * a.sizeA[k];
            pairImage(a, x, y);
            inB = pairQueryPoint(tB, y, eval) < a.isoB;
        }
        if (pairPredicate(a.op, inA, inB)) {
            integrateBoxMoments(vs, p, ss, m);
            for (int k = 0; k < 10; ++k) row[kIntM0 + k] = row[kIntM0 + k] + m[k];
        }
    }
}

// IntegratePair on the calling thread over the host arrays of tA and tB (integrate_pair_host.cpp)
int hostIntegratePair(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const PairArgs& p, const IntegrateArgs& a, hpsdf_integral* out,
                      hpsdf_integrate_cell** outCells, uint64_t* outCount);

}  // namespace hpsdf
