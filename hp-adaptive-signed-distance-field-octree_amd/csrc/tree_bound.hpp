// What a tree can prove about a whole region (include/hpsdf.h, "sparse ExtractSurface" and "QueryBounds"): the per-leaf constants G_x, G_y,
// G_z, S (leafBound), the monotone child selection of a walk that carries a range instead of a point (childMask), the view of a tree
// such a walk reads (ClsTree), and the walk of QueryBounds itself (boundsWalk).  Shared by surface_sparse.hip (classifyBlock), by
// query_bounds.hip (the kernels) and by host_query.cpp (the rows answered on the calling thread and the *_block entries): one set of
// statements with a fixed association, built with -ffp-contract=off, so host and device give the same bits.
//
// The part above "#ifdef __HIPCC__" is plain C++ (the device-free entries and the sanitizer builds compile it without a HIP compiler);
// below it are the device-side evaluation functor and the two kernels that make the constants of a device tree.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "block.hpp"
#include "device_types.hpp"
#include "lattice_check.hpp"
#include "runtime.hpp"
#include "tables.hpp"

namespace hpsdf {

constexpr int kLevels = HPSDF_TREE_MAX_DEPTH + 2;
constexpr double kClip = 1.0 + 1.0 / 16384.0;  // 1 + E, E = 2^-14 (include/hpsdf.h)

// What the walk reads of a tree: the 8-byte records, the line-aligned coefficients, 4 constants per node, the root map.
struct ClsTree {
    const NodeRec* nodes;
    const double* coeffs;
    const double* consts;  // per node: G_x, G_y, G_z, S (zeros for interior nodes)
    double rootCentre[3], rootInvSizes[3];
};

// G_a and S of one leaf (include/hpsdf.h): sums of non-negative terms, in row order
__host__ __device__ inline void leafBound(const double* __restrict__ c, uint32_t count, int depth, const double* __restrict__ nl,
                                          const uint8_t (*__restrict__ bidx)[4], double* __restrict__ out) {
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, s = 0.0;
    for (uint32_t r = 0; r < count; ++r) {
        const uint32_t k0 = bidx[r][0], k1 = bidx[r][1], k2 = bidx[r][2];
        double w = fabs(c[r]);
        w = w * nl[k0 * 11 + depth];
        w = w * nl[k1 * 11 + depth];
        w = w * nl[k2 * 11 + depth];
        s = s + w;
        g0 = g0 + w * (double)(k0 * (k0 + 1u) / 2u);
        g1 = g1 + w * (double)(k1 * (k1 + 1u) / 2u);
        g2 = g2 + w * (double)(k2 * (k2 + 1u) / 2u);
    }
    out[0] = g0, out[1] = g1, out[2] = g2, out[3] = s;
}

// children a walk with the range [pl, ph] must visit below a node centred at c: per axis the lower half if pl < c, the upper if ph >= c
__host__ __device__ inline uint32_t childMask(const double (&pl)[3], const double (&ph)[3], const double* c) {
    uint32_t m = 0xFFu;
    for (int a = 0; a < 3; ++a) {
        const uint32_t upper = a == 0 ? 0xAAu : (a == 1 ? 0xCCu : 0xF0u);  // children whose bit a is set
        if (!(pl[a] < c[a])) m &= upper;
        if (!(ph[a] >= c[a])) m &= ~upper;
    }
    return m;
}

// hostQueryPoint's statements (host_query.cpp): FApprox, Octree.cpp:859-901
struct HostEval {
    const Tables* T;
    double operator()(const double* c, int degree, double ux, double uy, double uz, int depth) const {
        const double u[3] = {ux, uy, uz};
        double tab[3][13];
        for (int a = 0; a < 3; ++a) {
            tab[a][0] = T->normalisedLengths[0][depth];
            double m2 = 0.0, m1 = 1.0;
            for (int j = 1; j <= degree; ++j) {
                const double l = T->recurrence[j][0] * u[a] * m1 - T->recurrence[j][1] * m2;
                m2 = m1, m1 = l;
                tab[a][j] = l * T->normalisedLengths[j][depth];
            }
        }
        double f = 0.0;
        const int n = (int)T->coeffCount[degree];
        for (int i = 0; i < n; ++i) {
            double lp = tab[0][T->basisIndex[i][0]];
            lp = lp * tab[1][T->basisIndex[i][1]];
            lp = lp * tab[2][T->basisIndex[i][2]];
            f = f + c[i] * lp;
        }
        return f;
    }
};

// a serialised block -> the arrays the walk reads: the query mirror (block.hpp) and the constants
struct HostTree {
    BlockMirror m;
    std::vector<double> consts;
    ClsTree view{};
};

inline int parseBlock(const void* block, size_t size, HostTree* out) {
    BlockView v;
    BlockMirror& m = out->m;
    const Tables& T = tables();
    {
        std::string why;
        int rc = readBlock(block, size, v, why);
        if (!rc) rc = mirrorBlock(v, T, m, why);
        if (rc) return fail(rc, why);
    }
    uint8_t bidx[kMaxCoeffs][4];
    for (int i = 0; i < kMaxCoeffs; ++i)
        for (int k = 0; k < 3; ++k) bidx[i][k] = (uint8_t)T.basisIndex[i][k];
    out->consts.assign(4 * (size_t)v.nNodes, 0.0);
    for (const uint64_t i : m.walk.order) {
        const NodeRec rec = m.recs[i];
        if (rec.b <= 12u && m.walk.depthOf[i] <= HPSDF_TREE_MAX_DEPTH)
            leafBound(m.padded.data() + rec.a, (uint32_t)T.coeffCount[rec.b], m.walk.depthOf[i], &T.normalisedLengths[0][0], bidx,
                      out->consts.data() + 4 * i);
    }
    out->view.nodes = m.recs.data();
    out->view.coeffs = m.padded.data();
    out->view.consts = out->consts.data();
    for (int a = 0; a < 3; ++a) out->view.rootCentre[a] = m.rootCentre[a], out->view.rootInvSizes[a] = m.rootInvSizes[a];
    return HPSDF_OK;
}

// ---- QueryBounds (include/hpsdf.h) ----------------------------------------------------------------------------------------------

// where a call's boxes come from: rows of six doubles, or the cells of a lattice (cell i + n0 (j + n1 k), corners by the surface
// lattice's arithmetic lo + (double)i * h, so neighbouring cells share their faces exactly); no box array is ever made of a lattice
struct BoxArray {
    const double* boxes;
    __host__ __device__ void get(size_t i, double (&a)[3], double (&b)[3]) const {
        for (int k = 0; k < 3; ++k) a[k] = boxes[6 * i + k], b[k] = boxes[6 * i + 3 + k];
    }
};
struct BoxGrid {
    double lo[3], h[3];
    uint32_t n[3];
    __host__ __device__ void get(size_t i, double (&a)[3], double (&b)[3]) const {
        const uint64_t r = (uint64_t)i / n[0];
        const uint32_t c[3] = {(uint32_t)((uint64_t)i - r * n[0]), (uint32_t)(r % n[1]), (uint32_t)(r / n[1])};
        for (int k = 0; k < 3; ++k) {
            a[k] = lo[k] + (double)c[k] * h[k];
            b[k] = lo[k] + (double)(c[k] + 1u) * h[k];
        }
    }
};

// the lattice arguments of hpsdf_query_bounds_grid_* (named `what`) -> the box source and the number of boxes
inline int checkBoundsGrid(const char* what, const double* rc, const double* ris, const double* lo, const double* hi, const uint32_t* n, BoxGrid* out,
                           size_t* count) {
    CheckedLattice cl{};
    if (const int r = checkLattice(what, kBoundsLimits, rc, ris, lo, hi, n, 0.0, &cl)) return r;
    if (cl.nCubes > (1ull << 32)) return fail(HPSDF_ERR_INVALID_ARGUMENT, std::string(what) + ": more than 2^32 boxes");
    for (int a = 0; a < 3; ++a) out->lo[a] = cl.lo[a], out->h[a] = cl.h[a], out->n[a] = cl.n[a];
    *count = (size_t)cl.nCubes;
    return HPSDF_OK;
}

struct BoundsRow {
    double lo, hi;
    uint32_t leaves;
    uint32_t status;
};

__host__ __device__ inline double boundsQuietNaN() { return __builtin_bit_cast(double, (unsigned long long)0x7FF8000000000000ull); }
__host__ __device__ inline double boundsInf() { return __builtin_bit_cast(double, (unsigned long long)0x7FF0000000000000ull); }
__host__ __device__ inline bool boundsFinite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

// the neighbouring double of a finite v on the side of +inf (up) or -inf
__host__ __device__ inline double boundsNeighbour(double v, bool up) {
    if (v == 0.0) return __builtin_bit_cast(double, up ? (unsigned long long)1ull : (unsigned long long)0x8000000000000001ull);
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return __builtin_bit_cast(double, (v > 0.0) == up ? b + 1ull : b - 1ull);
}

// An end of a sub-box's interval, f + d with d = -e or +e, rounded TOWARDS f: the double nearest to the exact sum among those between the
// exact sum and f (include/hpsdf.h, step 3).  s = fl(f + d); the error of an addition is a double, and Knuth's two-sum gives it exactly
// (six additions, no multiply-add to fuse): exact = s + err.  Where the addition rounded away from f -- below the exact sum for the lower
// end, above it for the upper end -- the end is s's neighbour on f's side.  An s that overflowed has err = NaN and stays infinite.
__host__ __device__ inline double boundsEnd(double f, double d) {
    const double s = f + d;
    const double dv = s - f;
    const double fv = s - dv;
    const double err = (f - fv) + (d - dv);
    if (d < 0.0 ? err > 0.0 : err < 0.0) return boundsNeighbour(s, d < 0.0);
    return s;
}

// The walk's stack on the calling thread: two small words per level.  (The kernels keep theirs in LDS, query_bounds.hip; the centre
// of the node a level holds is not stored at all: boundsWalk rebuilds it from the path.)
struct HostBoundsStack {
    uint32_t f[kLevels];
    uint8_t m[kLevels];
    uint32_t first(int d) const { return f[d]; }
    uint32_t mask(int d) const { return m[d]; }
    void setFirst(int d, uint32_t v) { f[d] = v; }
    void setMask(int d, uint32_t v) { m[d] = (uint8_t)v; }
};

// The interval of one box [a, b] (include/hpsdf.h, "QueryBounds", steps 1 to 4).  eval(c, degree, ux, uy, uz, depth): the leaf's polynomial
// as Query evaluates it -- called from ONE place, so the unrolled leaf code exists once per kernel.  Stack: first / mask per level.
// The centre of the node whose children are being visited is carried in three doubles: going down adds a quarter of the node's size per
// axis, coming back up takes the same dyadic off again (the child taken at each level is kept in three bits of `path`) -- every centre
// is a multiple of 2^-12 in [-0.5, 0.5], so both are exact and the centres are the ones classifyBlock keeps in its per-level array.
// boundsWalk is the map of step 1 followed by boundsWalkRange, the walk from a range [pl, ph] of the root's normalised frame that passed
// step 1's tests (IntegratePair enters there with a range it clamped itself, integrate_pair.hpp).
template <class Eval, class Stack>
__host__ __device__ inline void boundsWalkRange(const ClsTree& t, const double (&pl)[3], const double (&ph)[3], uint32_t subdiv, uint32_t maxLeaves,
                                                const Eval& eval, Stack& st, BoundsRow& R) {
    const double inf = boundsInf();
    double lo = inf, hi = -inf;
    uint32_t leaves = 0;
    int status = HPSDF_BOUNDS_OK;
    const uint32_t shift = subdiv >> 1;                // log2(subdiv) for 1, 2, 4
    const uint32_t cells = 1u << (3u * shift);         // sub-boxes of a leaf
    const double part = 1.0 / (double)subdiv;          // exact
    double cen[3] = {0.0, 0.0, 0.0};
    uint64_t path = 0;
    int depth = 0;
    st.setFirst(0, t.nodes[0].a);
    st.setMask(0, childMask(pl, ph, cen));
    while (depth >= 0) {
        const uint32_t m = st.mask(depth);
        if (m == 0) {
            if (--depth >= 0) {  // back to the centre of the node above
                const uint32_t up = (uint32_t)(path >> (3 * depth)) & 7u;
                const double q = 0.25 / (double)(1u << depth);
                for (int k = 0; k < 3; ++k) cen[k] = (up >> k) & 1u ? cen[k] - q : cen[k] + q;
            }
            continue;
        }
        const uint32_t ch = (uint32_t)__builtin_ctz(m);
        st.setMask(depth, m & (m - 1u));
        const double q = 0.25 / (double)(1u << depth);  // half the child's size: exact
        double cc[3];
        for (int k = 0; k < 3; ++k) cc[k] = (ch >> k) & 1u ? cen[k] + q : cen[k] - q;
        const uint32_t node = st.first(depth) + ch;
        const NodeRec rec = t.nodes[node];
        const int ld = depth + 1;  // the child's depth
        if (rec.b == kInteriorTag) {
            if (ld >= kLevels) {  // (no validated tree is this deep: nothing is claimed)
                status = HPSDF_BOUNDS_LEAF_LIMIT;
                break;
            }
            path = (path & ~(7ull << (3 * depth))) | ((uint64_t)ch << (3 * depth));
            depth = ld;
            st.setFirst(depth, rec.a);
            cen[0] = cc[0], cen[1] = cc[1], cen[2] = cc[2];
            st.setMask(depth, childMask(pl, ph, cc));
            continue;
        }
        if (leaves == maxLeaves || ld > HPSDF_TREE_MAX_DEPTH) {
            status = HPSDF_BOUNDS_LEAF_LIMIT;
            break;
        }
        ++leaves;
        const double s = (double)(2 << ld);
        double ua[3], w[3], ub[3];
        bool reached = true;
        for (int k = 0; k < 3; ++k) {
            double u0 = (pl[k] - cc[k]) * s, u1 = (ph[k] - cc[k]) * s;  // Octree.cpp:862 on the two extreme points
            u0 = u0 < -kClip ? -kClip : u0;
            u1 = u1 > kClip ? kClip : u1;
            if (!(u0 <= u1)) reached = false;  // no point of the box lies in this leaf
            ua[k] = u0, ub[k] = u1;
            w[k] = (u1 - u0) * part;
        }
        if (!reached) continue;
        const double* K = t.consts + 4 * (size_t)node;
        bool finite = true;
        for (uint32_t c = 0; c < cells; ++c) {  // x fastest, then y, then z
            const uint32_t idx[3] = {c & (subdiv - 1u), (c >> shift) & (subdiv - 1u), c >> (2u * shift)};
            double uc[3], rho[3];
            for (int k = 0; k < 3; ++k) {
                const double l = ua[k] + (double)idx[k] * w[k];
                const double h = idx[k] + 1u == subdiv ? ub[k] : ua[k] + (double)(idx[k] + 1u) * w[k];
                uc[k] = 0.5 * (l + h);
                rho[k] = 0.5 * (h - l);
            }
            const double fc = eval(t.coeffs + rec.a, (int)rec.b, uc[0], uc[1], uc[2], ld);
            const double e = HPSDF_SURFACE_SLACK * ((rho[0] * K[0] + rho[1] * K[1]) + rho[2] * K[2]) + HPSDF_SURFACE_ETA * K[3];
            if (!(boundsFinite(fc) && boundsFinite(e))) {
                finite = false;
                break;
            }
            const double el = boundsEnd(fc, -e), eh = boundsEnd(fc, e);
            if (el < lo) lo = el;
            if (eh > hi) hi = eh;
        }
        if (!finite) {
            status = HPSDF_BOUNDS_NOT_FINITE;
            break;
        }
    }
    if (status != HPSDF_BOUNDS_OK) lo = -inf, hi = inf;
    R.lo = lo, R.hi = hi, R.leaves = leaves, R.status = (uint32_t)status;
}

template <class Eval, class Stack>
__host__ __device__ inline void boundsWalk(const ClsTree& t, const double (&a)[3], const double (&b)[3], uint32_t subdiv, uint32_t maxLeaves,
                                           const Eval& eval, Stack& st, BoundsRow& R) {
    R.lo = R.hi = boundsQuietNaN(), R.leaves = 0, R.status = HPSDF_BOUNDS_INVALID;
    double pl[3], ph[3];
    bool valid = true;
    for (int k = 0; k < 3; ++k) {
        pl[k] = (a[k] - t.rootCentre[k]) * t.rootInvSizes[k];
        ph[k] = (b[k] - t.rootCentre[k]) * t.rootInvSizes[k];
        const float fl = (float)pl[k], fh = (float)ph[k];
        if (!(fl >= -0.5f && fl <= 0.5f && fh >= -0.5f && fh <= 0.5f)) valid = false;  // a corner fails Query's containment test (NaN too)
        if (!(pl[k] <= ph[k])) valid = false;
    }
    if (!valid) return;
    boundsWalkRange(t, pl, ph, subdiv, maxLeaves, eval, st, R);
}

// n rows on the calling thread (host_query.cpp): the kernels' rows bit for bit.  boxes == nullptr: the cells of *grid.  leaves may be null.
void hostBoundsRows(const ClsTree& t, const double* boxes, const BoxGrid* grid, size_t n, uint32_t subdiv, uint32_t maxLeaves, double* lo, double* hi,
                    uint8_t* status, uint32_t* leaves);
// what hpsdf_query_bounds_* reject before anything runs (0: fine); in: the box array, or the lattice arguments of the grid entries
int boundsArgumentError(uint32_t subdiv, uint32_t maxLeaves, size_t n, const void* in, const void* lo, const void* hi, const void* status);

}  // namespace hpsdf

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "leaf_eval.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kConstsThreads = 256;

template <int MAXP>
struct DevEval {
    const double* sNl;
    const double* sRec;
    __device__ double operator()(const double* c, int degree, double ux, double uy, double uz, int depth) const {
        return evalLeaf<MAXP>(c, degree, ux, uy, uz, depth, sNl, sRec);
    }
};

// depth[i] of every node, handed down from the root level by level by ONE workgroup (a node's record does not hold it)
__global__ __launch_bounds__(1024) void leaf_depth_kernel(const NodeRec* __restrict__ nodes, uint32_t nNodes, int maxDepth, uint8_t* depth) {
    for (uint32_t i = threadIdx.x; i < nNodes; i += 1024u) depth[i] = i == 0 ? 0 : 0xFF;
    __syncthreads();
    for (int level = 0; level < maxDepth; ++level) {
        for (uint32_t i = threadIdx.x; i < nNodes; i += 1024u) {
            const NodeRec rec = nodes[i];
            if (depth[i] == level && rec.b == kInteriorTag && rec.a < nNodes && nNodes - rec.a >= 8u)
                for (uint32_t c = 0; c < 8u; ++c) depth[rec.a + c] = (uint8_t)(level + 1);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kConstsThreads) void leaf_consts_kernel(const NodeRec* __restrict__ nodes, const double* __restrict__ coeffs,
                                                                    const uint8_t* __restrict__ depth, uint32_t nNodes,
                                                                    const DeviceTables* __restrict__ T, double* __restrict__ consts) {
    const uint32_t i = blockIdx.x * kConstsThreads + threadIdx.x;
    if (i >= nNodes) return;
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    const NodeRec rec = nodes[i];
    const int d = depth[i];
    if (rec.b <= 12u && d <= HPSDF_TREE_MAX_DEPTH) leafBound(coeffs + rec.a, T->count[rec.b], d, &T->nl[0][0], T->bidx, out);
    for (int k = 0; k < 4; ++k) consts[4 * (size_t)i + k] = out[k];
}

// the constants of a device tree's leaves into dConsts (4 doubles a node), with dDepth (a byte a node) as scratch; not synchronised
inline hipError_t launchLeafConsts(hipStream_t s, const hpsdf_tree* t, const DeviceTables* dTables, uint8_t* dDepth, double* dConsts) {
    const uint32_t nNodes = (uint32_t)t->nNodes;
    hipLaunchKernelGGL(leaf_depth_kernel, dim3(1), dim3(1024), 0, s, t->dev.nodes, nNodes, t->maxDepth, dDepth);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(leaf_consts_kernel, dim3((nNodes + kConstsThreads - 1) / kConstsThreads), dim3(kConstsThreads), 0, s, t->dev.nodes,
                       t->dev.coeffs, dDepth, nNodes, dTables, dConsts);
    return hipGetLastError();
}

}  // namespace

}  // namespace hpsdf
#endif
