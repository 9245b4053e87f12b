// Dual contouring's vertex (include/hpsdf.h, "ExtractSurfaceDual"): from the Hermite samples of a mixed cube's crossing edges -- the
// marching-cubes vertex p_e of the edge, and QueryGradient's value f_e and gradient g_e there -- the point that minimises
// sum_e (f_e + g_e . (x - p_e) - iso)^2 over the well-determined directions of A = sum g_e g_e^T, clamped into the cube.
//
// One set of statements for the calling thread (host_query.cpp, hpsdf_extract_surface_dual_block) and the kernels (surface_dual.hip):
// the mean, the accumulation of one sample, the Jacobi sweeps, the truncated solve and the clamp.  Only +, -, *, / and sqrt, all
// correctly rounded on both sides and built with -ffp-contract=off, so both sides give the same bits.  Every loop has a fixed trip
// count: a lane's solve costs what its neighbour's does.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/hpsdf.h"
#include "leaf_jet.hpp"

namespace hpsdf {

// what the Hermite kernel leaves for a crossing edge, one 64-byte line: p_e, f_e, g_e (not normalised)
struct alignas(64) DualRecord {
    double p[3], f, g[3], pad;
};
static_assert(sizeof(DualRecord) == 64, "one line per record");

// A (symmetric, both halves kept) and b of a cube's normal equations
struct DualNormal {
    double a[3][3], b[3];
};

__host__ __device__ inline bool dualFinite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

__host__ __device__ inline void dualClear(DualNormal& N, double (&sum)[3]) {
    for (int r = 0; r < 3; ++r) {
        N.b[r] = 0.0, sum[r] = 0.0;
        for (int c = 0; c < 3; ++c) N.a[r][c] = 0.0;
    }
}

// pass 1, once per crossing edge in cube-local order: sum = sum + p_e; then m = sum / k
__host__ __device__ inline void dualAddPoint(const double* p, double (&sum)[3]) {
    for (int a = 0; a < 3; ++a) sum[a] = sum[a] + p[a];
}
__host__ __device__ inline void dualMean(const double (&sum)[3], uint32_t k, double (&m)[3]) {
    for (int a = 0; a < 3; ++a) m[a] = sum[a] / (double)k;
}

// pass 2, once per crossing edge in the same order: d = p_e - m, r = (iso - f_e) + sum3(g_e . d), A += g g^T, b += g r
__host__ __device__ inline void dualAccumulate(const double* p, double f, const double* g, const double (&m)[3], double iso, int leftAssoc,
                                               DualNormal& N) {
    const double d[3] = {p[0] - m[0], p[1] - m[1], p[2] - m[2]};
    const double r = (iso - f) + sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], leftAssoc);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N.a[i][j] = N.a[i][j] + g[i] * g[j];
        N.b[i] = N.b[i] + g[i] * r;
    }
}

// One Jacobi rotation of the pair (P, Q), R being the third index; skipped when the off-diagonal entry is exactly 0.
// theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (sgn(0) = 1), c = 1 / sqrt(t^2 + 1), s = t c.
template <int P, int Q, int R>
__host__ __device__ inline void dualRotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// HPSDF_DUAL_SWEEPS cyclic sweeps over (0,1), (0,2), (1,2): a's diagonal becomes the eigenvalues, v's columns the eigenvectors
__host__ __device__ inline void dualJacobi(double (&a)[3][3], double (&v)[3][3]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < HPSDF_DUAL_SWEEPS; ++sweep) {
        dualRotate<0, 1, 2>(a, v);
        dualRotate<0, 2, 1>(a, v);
        dualRotate<1, 2, 0>(a, v);
    }
}

// The vertex of a cube from its normal equations and mean point m: the truncated solve, the fall-back to m, the clamp into the
// cube's closed range [cubeLo, cubeHi].  Returns the info byte: the rank in bits 0-1, HPSDF_DUAL_CLAMPED if an axis was clamped.
__host__ __device__ inline uint32_t dualSolve(DualNormal& N, const double (&m)[3], double tau, int leftAssoc, const double (&cubeLo)[3],
                                              const double (&cubeHi)[3], double (&x)[3]) {
    double v[3][3];
    dualJacobi(N.a, v);
    const double l[3] = {N.a[0][0], N.a[1][1], N.a[2][2]};
    double lmax = l[0];
    if (l[1] > lmax) lmax = l[1];
    if (l[2] > lmax) lmax = l[2];
    uint32_t rank = 0;
    x[0] = m[0], x[1] = m[1], x[2] = m[2];
    if (lmax > 0.0 && dualFinite(lmax)) {
        const double thr = tau * lmax;
        for (int i = 0; i < 3; ++i) {
            if (!(l[i] > thr && l[i] > 0.0)) continue;
            const double w = sum3(v[0][i] * N.b[0], v[1][i] * N.b[1], v[2][i] * N.b[2], leftAssoc) / l[i];
            for (int a = 0; a < 3; ++a) x[a] = x[a] + v[a][i] * w;
            ++rank;
        }
        if (!(dualFinite(x[0]) && dualFinite(x[1]) && dualFinite(x[2]))) {
            x[0] = m[0], x[1] = m[1], x[2] = m[2];
            rank = 0;
        }
    }
    uint32_t info = rank;
    for (int a = 0; a < 3; ++a) {
        if (x[a] < cubeLo[a]) x[a] = cubeLo[a], info |= HPSDF_DUAL_CLAMPED;
        if (x[a] > cubeHi[a]) x[a] = cubeHi[a], info |= HPSDF_DUAL_CLAMPED;
    }
    return info;
}

// ---- the lattice's topology, shared by both sides ---------------------------------------------------------------------------------

// Cube-local edge e of the cube whose lower corner is lattice point (i, j, k): the lower point's offset (dx, dy, dz) and the axis
// (surface_table.hpp's numbering: x edges 0..3, y 4..7, z 8..11; lower corners 0 2 4 6 | 0 1 4 5 | 0 1 2 3)
__host__ __device__ inline uint32_t dualEdgeCorner(uint32_t e) { return e < 4u ? 2u * e : (e < 8u ? (e - 4u) + ((e - 4u) & 2u) : e - 8u); }
__host__ __device__ inline uint32_t dualEdgeAxis(uint32_t e) { return e >> 2; }

// The four cubes around an interior edge along axis a at lattice point idx, counter-clockwise seen from +a: (b, c) offsets
// (-1,-1), (0,-1), (0,0), (-1,0) with b = (a + 1) % 3, c = (a + 2) % 3.  Q = i + n0 (j + n1 k).
__host__ __device__ inline void dualQuadCubes(const uint32_t (&idx)[3], uint32_t a, const uint32_t* n, uint32_t (&Q)[4]) {
    const uint32_t b = (a + 1u) % 3u, c = (a + 2u) % 3u;
    const uint32_t ob[4] = {1u, 0u, 0u, 1u}, oc[4] = {1u, 1u, 0u, 0u};
    for (int q = 0; q < 4; ++q) {
        uint32_t id[3];
        id[a] = idx[a], id[b] = idx[b] - ob[q], id[c] = idx[c] - oc[q];
        Q[q] = id[0] + n[0] * (id[1] + n[1] * id[2]);
    }
}
__host__ __device__ inline bool dualInterior(const uint32_t (&idx)[3], uint32_t a, const uint32_t* n) {
    const uint32_t b = (a + 1u) % 3u, c = (a + 2u) % 3u;
    return idx[b] >= 1u && idx[b] <= n[b] - 1u && idx[c] >= 1u && idx[c] <= n[c] - 1u;
}

}  // namespace hpsdf
