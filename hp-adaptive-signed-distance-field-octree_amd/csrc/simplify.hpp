// Simplify (include/hpsdf.h, "Simplify"): the statements the host path (simplify_host.cpp) and the device path (simplify.hip) share -- the
// three one-axis passes of a child into its parent and back, the residual and its reduction rule, the bound, the decision, the tail
// energies -- and the one routine that makes the output block from the per-node results.  Every float64 sum has its order written here:
// a dot product runs over its index ascending from 0.0, the children are taken 0 .. 7, the squares are reduced by simpReduce's tree.
// Built with -ffp-contract=off like every other unit, so both paths give the same bytes.  Plain C++ apart from the function attributes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "block.hpp"
#include "tables.hpp"

namespace hpsdf {

constexpr int kSimpQ = kMaxDegree + 1;    // entries per axis of the largest cube, and the row length of a transfer matrix
constexpr uint32_t kSimpFlags = HPSDF_SIMPLIFY_MERGE | HPSDF_SIMPLIFY_TRUNCATE;

// The entries (i, j, k), i + j + k <= q, in the basis's graded order: entry e is row e of the basis.  A leaf of degree d stores the first
// count[d] of them; count[6] is 83, not 84 (tables.hpp), so entry 83 = (6, 0, 0) of a degree-6 leaf is not stored and counts as 0.
__host__ __device__ inline uint32_t simpEntries(uint32_t q) { return (q + 1u) * (q + 2u) * (q + 3u) / 6u; }
__host__ __device__ inline uint32_t simpPow2(uint32_t n) {
    uint32_t p = 1u;
    while (p < n) p <<= 1;
    return p;
}
// volume of a cell at `depth` in the root's frame (depth <= 11: exact)
__host__ __device__ inline double simpVolume(uint32_t depth) { return 1.0 / (double)(1ull << (3u * depth)); }

// sum over i = 0 .. a of Th[a][i] * in[i * stride]
__host__ __device__ inline double simpUp(const double* Th, const double* in, int stride, int a) {
    double s = 0.0;
    for (int i = 0; i <= a; ++i) s = s + Th[a * kSimpQ + i] * in[i * stride];
    return s;
}
// sum over a = i .. hi of Th[a][i] * in[a * stride]
__host__ __device__ inline double simpDown(const double* Th, const double* in, int stride, int i, int hi) {
    double s = 0.0;
    for (int a = i; a <= hi; ++a) s = s + Th[a * kSimpQ + i] * in[a * stride];
    return s;
}

// Cubes of Q^3 doubles, entry (x, y, z) at (x Q + y) Q + z; only the entries with x + y + z <= q are ever written or read.
// Child -> parent, child octant n (bit a of n: the upper half on axis a): U holds the child's entries c[i, j, k];
//   X:  V[a, j, k] = sum_{i <= a} T_sx[a][i] U[i, j, k]      Y:  U[a, b, k] = sum_{j <= b} T_sy[b][j] V[a, j, k]
//   Z:  parent[a, b, c] += sum_{k <= c} T_sz[c][k] U[a, b, k]
// Parent -> child (the parent's polynomial restricted to the octant): U holds the parent's entries;
//   Z': V[a, b, k] = sum_{c = k .. q-a-b} T_sz[c][k] U[a, b, c]    Y': U[a, j, k] = sum_{b = j .. q-a-k} T_sy[b][j] V[a, b, k]
//   X': r[i, j, k] = sum_{a = i .. q-j-k} T_sx[a][i] U[a, j, k]
template <int Q>
struct SimpCube {
    static __host__ __device__ int at(int x, int y, int z) { return (x * Q + y) * Q + z; }
    static __host__ __device__ double fwdX(const double* T, uint32_t n, const double* U, int a, int j, int k) {
        return simpUp(T + (n & 1u) * (kSimpQ * kSimpQ), U + at(0, j, k), Q * Q, a);
    }
    static __host__ __device__ double fwdY(const double* T, uint32_t n, const double* V, int a, int b, int k) {
        return simpUp(T + ((n >> 1) & 1u) * (kSimpQ * kSimpQ), V + at(a, 0, k), Q, b);
    }
    static __host__ __device__ double fwdZ(const double* T, uint32_t n, const double* U, int a, int b, int c) {
        return simpUp(T + ((n >> 2) & 1u) * (kSimpQ * kSimpQ), U + at(a, b, 0), 1, c);
    }
    static __host__ __device__ double bwdZ(const double* T, uint32_t n, const double* U, int q, int a, int b, int k) {
        return simpDown(T + ((n >> 2) & 1u) * (kSimpQ * kSimpQ), U + at(a, b, 0), 1, k, q - a - b);
    }
    static __host__ __device__ double bwdY(const double* T, uint32_t n, const double* V, int q, int a, int j, int k) {
        return simpDown(T + ((n >> 1) & 1u) * (kSimpQ * kSimpQ), V + at(a, 0, k), Q, j, q - a - k);
    }
    static __host__ __device__ double bwdX(const double* T, uint32_t n, const double* U, int q, int i, int j, int k) {
        return simpDown(T + (n & 1u) * (kSimpQ * kSimpQ), U + at(0, j, k), Q * Q, i, q - j - k);
    }
};

// The reduction rule of the residual: acc holds simpPow2(entries) numbers -- entry e's squares summed over the children 0 .. 7, zero
// from `entries` on --; for stride = half, half / 2, ..., 1: acc[t] = acc[t] + acc[t + stride] for t < stride.  The sum ends in acc[0].
// (The kernel runs the same steps with its lanes as t.)
inline double simpReduce(double* acc, uint32_t p2) {
    for (uint32_t stride = p2 >> 1; stride > 0; stride >>= 1)
        for (uint32_t t = 0; t < stride; ++t) acc[t] = acc[t] + acc[t + stride];
    return acc[0];
}

// b = (sqrt(step) + sqrt(carried))^2: the triangle inequality in L2 over the cell, `carried` the e of what is already there
__host__ __device__ inline double simpBound(double step, double carried) {
    const double r = sqrt(step) + sqrt(carried);
    return r * r;
}
// b <= rms^2 vol(depth), and b finite: a NaN fails both comparisons
__host__ __device__ inline bool simpAccept(double b, double rms, uint32_t depth) { return b <= (rms * rms) * simpVolume(depth) && b <= DBL_MAX; }

// Truncation of one leaf (rows c, degree d, at `depth`, carrying *e): the tail of degree d'' is the sum of the squares of the rows from
// count[d''] on, formed shell by shell from the top -- a shell's squares in row order, tail = tail + shell --; the degree goes down
// while the bound is accepted and stops at the first that is not.  Returns the new degree; *e becomes its bound.
template <class Count>
__host__ __device__ inline uint32_t simpTruncate(const double* c, uint32_t d, const Count* count, double rms, uint32_t depth, double* e) {
    const double carried = *e;
    double tail = 0.0;
    uint32_t keep = d;
    for (uint32_t dd = d; dd-- > 0u;) {
        double shell = 0.0;
        for (uint32_t r = (uint32_t)count[dd]; r < (uint32_t)count[dd + 1u]; ++r) shell = shell + c[r] * c[r];
        tail = tail + shell;
        const double b = simpBound(tail, carried);
        if (!simpAccept(b, rms, depth)) break;
        keep = dd;
        *e = b;
    }
    return keep;
}

// ---- the per-node results of both paths, and the block made from them (host only from here on)

// A node as the passes leave it.  rowsAt < nCoeffs: the rows lie in the source block's store; otherwise at rowsAt - nCoeffs of `ext`,
// the rows the merges made.
struct SimpNode {
    uint64_t rowsAt;
    double e;
    uint32_t child;   // first child in the source (interior nodes of the source; a merged node keeps it)
    uint8_t degree;   // 13: interior
    uint8_t depth;
    uint8_t srcDegree;  // what the source said
    uint8_t pad;
};
static_assert(sizeof(SimpNode) == 24, "uploaded and downloaded as it is");

struct SimpState {
    std::vector<SimpNode> nodes;              // per source node
    std::vector<std::vector<uint32_t>> level; // level[d]: the source's interior nodes at depth d, in increasing index
    std::vector<double> ext;
    uint64_t extBound = 0;                    // no run of the merge pass makes more rows than this
    uint64_t levels = 0, truncations = 0;
};

// What hpsdf_simplify* reject before anything runs (0: fine)
int simplifyArgumentError(double rms, uint32_t flags, const void* outBlock, const void* outSize);

// The state a run starts from: every reached leaf with its rows in the source and e = 0.
inline void simplifyBegin(const BlockView& v, const BlockMirror& m, const Tables& T, SimpState& s) {
    s.nodes.assign(v.nNodes, SimpNode{0, 0.0, 0, 0xFF, 0, 0xFF, 0});
    s.level.assign((size_t)m.walk.maxDepth + 1, {});
    for (uint64_t i = 0; i < v.nNodes; ++i) {
        if (!m.walk.reached[i]) continue;
        const hpsdf_node& n = v.nodes[i];
        SimpNode& o = s.nodes[i];
        o.degree = o.srcDegree = n.degree;
        o.depth = m.walk.depthOf[i];
        if (n.degree == kInteriorDegree) {
            o.child = (uint32_t)n.child_idx;
            if (o.depth < s.level.size()) s.level[o.depth].push_back((uint32_t)i);
        } else {
            o.rowsAt = n.coeffs_start;
        }
    }
    // an interior node can be given at most the rows of the largest degree below it
    std::vector<uint8_t> top(v.nNodes, 0);
    s.extBound = 0;
    for (size_t k = m.walk.order.size(); k-- > 0;) {  // (a parent is popped before its children: backwards, children come first)
        const uint64_t i = m.walk.order[k];
        const hpsdf_node& n = v.nodes[i];
        if (n.degree != kInteriorDegree) {
            top[i] = n.degree;
            continue;
        }
        for (unsigned c = 0; c < 8; ++c) top[i] = top[i] > top[n.child_idx + c] ? top[i] : top[n.child_idx + c];
        if (i != 0) s.extBound += T.coeffCount[top[i]];
    }
}

// The passes over a state simplifyBegin made: on the calling thread (simplify_host.cpp), and on ctx's device (simplify.hip: HPSDF_OK or
// the failure's status with its message set).  Both leave the same degrees, e and rows.
void simplifyOnHost(const BlockView& v, const BlockMirror& m, const Tables& T, double rms, uint32_t flags, SimpState& s);
int simplifyOnDevice(hpsdf_ctx* ctx, const BlockView& v, const BlockMirror& m, double rms, uint32_t flags, SimpState& s);

// The surviving leaves in increasing index: those a walk from the root reaches through the nodes that are still interior.
inline void simplifyLeaves(const SimpState& s, std::vector<uint32_t>& leaves) {
    std::vector<uint8_t> alive(s.nodes.size(), 0);
    std::vector<uint32_t> stack{0u};
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        alive[i] = 1;
        if (s.nodes[i].degree == kInteriorDegree)
            for (uint32_t c = 0; c < 8u; ++c) stack.push_back(s.nodes[i].child + c);
    }
    leaves.clear();
    for (size_t i = 0; i < s.nodes.size(); ++i)
        if (alive[i] && s.nodes[i].degree != kInteriorDegree) leaves.push_back((uint32_t)i);
}

// The output block (include/hpsdf.h, "Simplify", "Output"): the surviving nodes in their old order with child_idx remapped, boxes and
// depths as in the source, the coefficients in the order of a depth-first walk with children 0 .. 7 (Octree::ReallocCoeffs,
// Octree.cpp:474-555), the Config copied.  `alloc` hands out the block's memory (nullptr from it: HPSDF_ERR_OUT_OF_MEMORY).
template <class Alloc>
int simplifyAssemble(const BlockView& v, const Tables& T, const SimpState& s, Alloc&& alloc, void** outBlock, size_t* outSize,
                     hpsdf_simplify_stats* stats, std::string& err) {
    const size_t nn = s.nodes.size();
    std::vector<uint8_t> alive(nn, 0);
    std::vector<uint32_t> dfs;  // the surviving leaves in walk order
    hpsdf_simplify_stats st;
    std::memset(&st, 0, sizeof st);
    {
        std::vector<uint32_t> stack{0u};
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            stack.pop_back();
            alive[i] = 1;
            if (s.nodes[i].degree == kInteriorDegree)
                for (uint32_t c = 8u; c-- > 0u;) stack.push_back(s.nodes[i].child + c);  // (child 0 is popped first)
            else
                dfs.push_back(i);
        }
    }
    std::vector<uint64_t> rank(nn, 0), start(nn, 0);
    uint64_t nNodes = 0, nCoeffs = 0;
    for (size_t i = 0; i < nn; ++i) {
        rank[i] = nNodes;
        nNodes += alive[i];
        if (s.nodes[i].srcDegree == 0xFF) continue;  // (not reached in the source)
        st.nodes_in += 1;
        if (s.nodes[i].srcDegree != kInteriorDegree) {
            st.leaves_in += 1;
            st.coeffs_in += T.coeffCount[s.nodes[i].srcDegree];
        } else if (s.nodes[i].degree != kInteriorDegree) {
            st.merges += 1;
        }
    }
    for (const uint32_t i : dfs) {
        start[i] = nCoeffs;
        nCoeffs += T.coeffCount[s.nodes[i].degree];
    }
    const size_t bytes = blockBytes(nCoeffs, nNodes);
    uint8_t* p = (uint8_t*)alloc(bytes);
    if (!p) {
        err = "hpsdf_simplify: out of memory (the output block)";
        return HPSDF_ERR_OUT_OF_MEMORY;
    }
    std::memcpy(p, &nCoeffs, 8);
    double* coeffs = (double*)(p + kBlockCoeffsAt);
    for (const uint32_t i : dfs) {
        const SimpNode& n = s.nodes[i];
        const double* rows = n.rowsAt < v.nCoeffs ? v.coeffs + n.rowsAt : s.ext.data() + (n.rowsAt - v.nCoeffs);
        if (T.coeffCount[n.degree]) std::memcpy(coeffs + start[i], rows, 8 * (size_t)T.coeffCount[n.degree]);
        st.error_bound = st.error_bound + n.e;
        const double cell = sqrt(n.e / simpVolume(n.depth));
        if (cell > st.max_cell_rms) st.max_cell_rms = cell;
    }
    std::memcpy(p + blockNodeCountAt(nCoeffs), &nNodes, 8);
    uint8_t* nodesAt = p + blockNodesAt(nCoeffs);
    for (size_t i = 0; i < nn; ++i) {
        if (!alive[i]) continue;
        hpsdf_node n = v.nodes[i];
        if (s.nodes[i].degree == kInteriorDegree) {
            n.child_idx = rank[n.child_idx];
        } else {
            n.child_idx = ~0ull;
            n.degree = s.nodes[i].degree;
            n.coeffs_start = start[i];
        }
        std::memcpy(nodesAt + sizeof(hpsdf_node) * rank[i], &n, sizeof n);
    }
    std::memcpy(p + blockConfigAt(nCoeffs, nNodes), &v.cfg, sizeof v.cfg);
    st.nodes_out = nNodes, st.coeffs_out = nCoeffs, st.leaves_out = dfs.size();
    st.levels = s.levels, st.truncations = s.truncations;
    *outBlock = p, *outSize = bytes;
    if (stats) *stats = st;
    return HPSDF_OK;
}

}  // namespace hpsdf
