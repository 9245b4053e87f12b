// hpsdf_extract_surface_sparse: hpsdf_extract_surface's mesh, bit for bit, evaluated only in the blocks of 8^3 cubes the tree cannot
// rule out (include/hpsdf.h states the blocks, the classes, the bound and the derivation of its slack).  What must equal the dense
// call's -- case table, vertex arithmetic, wave helpers, argument checks -- is surface_common.hpp's, included by both.
//
//   1. leaf_depth_kernel / leaf_consts_kernel (tree_bound.hpp, shared with QueryBounds): per leaf G_x, G_y, G_z, S (leafBound) -- the
//      depth of a node is not in the 8-byte mirror, one workgroup hands it down level by level;
//   2. sparse_classify_kernel: one lane per block walks the tree with the block's two extreme lattice points (classifyBlock: the very
//      function hpsdf_surface_classify_host runs on the calling thread, so both give the same bytes);
//   3. rocPRIM reduce + select: the class-0 blocks in block order;
//   4. sparse_block_kernel<COUNT>: one workgroup per active block -- its <= 9^3 values through Query's queryPoint into LDS, ballots of
//      the crossing edges it owns and its cubes' triangle counts from the case table;  rocPRIM exclusive scans of both;
//   5. sparse_block_kernel<EMIT>: the values again (5.8 KB a block is not stored), then vertex records (edge id, xyz) and triangle
//      records (key 8 Q + index in the cube, three edge ids) at the prefixes;
//   6. rocPRIM radix sorts of (edge id, record) and (key, record); sparse_gather_kernel puts the vertices in edge-id order and
//      sparse_renumber_kernel replaces a triangle's edge ids by their ranks among the sorted vertex keys (binary search): the dense
//      call's numbering, with no neighbour logic.
// No atomics on anything that reaches the output (one counter of visited leaves for the statistics).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "block.hpp"
#include "device_types.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "surface_common.hpp"
#include "tables.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

constexpr uint32_t kB = HPSDF_SURFACE_BLOCK;  // cubes per axis of a block
constexpr uint32_t kP = kB + 1;               // points per axis of its closed range
constexpr uint32_t kBlockPts = kP * kP * kP;  // 729
constexpr uint32_t kBlockCubes = kB * kB * kB;
constexpr uint32_t kEdgeRounds = (3 * kBlockPts + kSurfThreads - 1) / kSurfThreads;  // 9
constexpr uint32_t kCubeRounds = kBlockCubes / kSurfThreads;                     // 2

struct SparseLattice {
    double lo[3], h[3];
    uint32_t n[3], nb[3];
    uint64_t np[3];  // points per axis
    uint64_t nBlocks;
};

// The class of block b (include/hpsdf.h).  eval(c, degree, ux, uy, uz, depth): the leaf's polynomial as Query evaluates it.
template <class Eval>
__host__ __device__ inline uint8_t classifyBlock(const ClsTree& t, const SparseLattice& g, double iso, uint64_t b, const Eval& eval,
                                                 uint32_t& visited) {
    visited = 0;
    const uint64_t r = b / g.nb[0];
    const uint32_t bi[3] = {(uint32_t)(b - r * g.nb[0]), (uint32_t)(r % g.nb[1]), (uint32_t)(r / g.nb[1])};
    double pl[3], ph[3];
    for (int a = 0; a < 3; ++a) {
        const uint32_t i0 = kB * bi[a], i1 = i0 + kB < g.n[a] ? i0 + kB : g.n[a];
        const double xl = g.lo[a] + (double)i0 * g.h[a], xh = g.lo[a] + (double)i1 * g.h[a];
        pl[a] = (xl - t.rootCentre[a]) * t.rootInvSizes[a];
        ph[a] = (xh - t.rootCentre[a]) * t.rootInvSizes[a];
        const float fl = (float)pl[a], fh = (float)ph[a];
        if (!(fl >= -0.5f && fl <= 0.5f && fh >= -0.5f && fh <= 0.5f)) return 0;  // a corner fails Query's containment test
        if (!(pl[a] <= ph[a])) return 0;
    }
    if (t.nodes[0].b != kInteriorTag) return 0;
    uint32_t first[kLevels];
    uint32_t mask[kLevels];
    double cen[kLevels][3];
    int depth = 0, sign = 0;
    first[0] = t.nodes[0].a;
    cen[0][0] = cen[0][1] = cen[0][2] = 0.0;
    mask[0] = childMask(pl, ph, cen[0]);
    while (depth >= 0) {
        const uint32_t m = mask[depth];
        if (m == 0) {
            --depth;
            continue;
        }
        const uint32_t ch = (uint32_t)__builtin_ctz(m);
        mask[depth] = m & (m - 1u);
        const double q = 0.25 / (double)(1u << depth);  // half the child's size: exact
        double cc[3];
        for (int a = 0; a < 3; ++a) cc[a] = (ch >> a) & 1u ? cen[depth][a] + q : cen[depth][a] - q;
        const uint32_t node = first[depth] + ch;
        const NodeRec rec = t.nodes[node];
        if (rec.b == kInteriorTag) {
            if (depth + 1 >= kLevels) return 0;
            ++depth;
            first[depth] = rec.a;
            cen[depth][0] = cc[0], cen[depth][1] = cc[1], cen[depth][2] = cc[2];
            mask[depth] = childMask(pl, ph, cc);
            continue;
        }
        const int ld = depth + 1;  // the leaf's depth
        if (++visited > (uint32_t)HPSDF_SURFACE_MAX_LEAVES || ld > HPSDF_TREE_MAX_DEPTH) return 0;
        const double s = (double)(2 << ld);
        double uc[3], rho[3];
        bool reached = true;
        for (int a = 0; a < 3; ++a) {
            double ua = (pl[a] - cc[a]) * s, ub = (ph[a] - cc[a]) * s;  // Octree.cpp:862 on the two extreme points
            ua = ua < -kClip ? -kClip : ua;
            ub = ub > kClip ? kClip : ub;
            if (!(ua <= ub)) reached = false;  // no point of the block lies in this leaf
            uc[a] = 0.5 * (ua + ub);
            rho[a] = 0.5 * (ub - ua);
        }
        if (!reached) continue;
        const double* K = t.consts + 4 * (size_t)node;
        const double bound = HPSDF_SURFACE_SLACK * ((rho[0] * K[0] + rho[1] * K[1]) + rho[2] * K[2]) + HPSDF_SURFACE_ETA * K[3];
        const double d = eval(t.coeffs + rec.a, (int)rec.b, uc[0], uc[1], uc[2], ld) - iso;
        int sg;
        if (d > bound)
            sg = 1;
        else if (-d > bound)
            sg = -1;
        else
            return 0;  // (a NaN lands here too)
        if (sign != 0 && sg != sign) return 0;
        sign = sg;
    }
    return sign == 0 ? 0 : (sign > 0 ? 1 : 2);
}

// ---- constants and classes -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kSurfThreads) void sparse_classify_kernel(ClsTree t, const DeviceTables* __restrict__ T, SparseLattice g, double iso,
                                                                   uint64_t firstBlock, uint64_t count, uint8_t* __restrict__ out,
                                                                   unsigned long long* __restrict__ visitedTotal) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<12> eval{sNl, sRec};
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; i < count; i += stride) {
        uint32_t visited;
        out[i] = classifyBlock(t, g, iso, firstBlock + i, eval, visited);
        mine += visited;
    }
    if (visitedTotal != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if ((threadIdx.x & 63u) == 0 && mine != 0) atomicAdd(visitedTotal, mine);
    }
}

// ---- the active blocks ---------------------------------------------------------------------------------------------------------

struct BlockOut {
    uint32_t* vcount;  // COUNT: per active block
    uint32_t* tcount;
    const uint64_t* vprefix;  // EMIT: exclusive prefixes of the two
    const uint64_t* tprefix;
    uint64_t* vkey;  // vertex records: edge id, own position, xyz
    uint64_t* vidx;
    double* vxyz;
    uint64_t* tkey;  // triangle records: 8 Q + index in the cube, own position, three edge ids
    uint64_t* tidx;
    uint64_t* tedge;
};

template <int MAXP, bool EMIT>
__global__ __launch_bounds__(kSurfThreads) void sparse_block_kernel(TreeDev t, const DeviceTables* __restrict__ T, SparseLattice g, double iso,
                                                                const uint64_t* __restrict__ active, uint64_t nActive, BlockOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint64_t sCase[256];
    __shared__ double sV[kBlockPts];
    __shared__ uint8_t sIn[kBlockPts + 7];
    __shared__ uint32_t sVW[4], sTW[kCubeRounds][4];
    stageQueryTables(T, sNl, sRec);
    stageCases(sCase);
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    for (uint64_t ab = blockIdx.x; ab < nActive; ab += gridDim.x) {
        __syncthreads();  // the tables are staged; the previous block's LDS is no longer read
        const uint64_t b = active[ab];
        const uint64_t br = b / g.nb[0];
        const uint32_t bi[3] = {(uint32_t)(b - br * g.nb[0]), (uint32_t)(br % g.nb[1]), (uint32_t)(br / g.nb[1])};
        uint32_t base[3], cnt[3], own[3];
        for (int a = 0; a < 3; ++a) {
            base[a] = kB * bi[a];
            cnt[a] = g.n[a] - base[a] < kB ? g.n[a] - base[a] : kB;  // cubes of the block on this axis
            own[a] = cnt[a] + (bi[a] + 1u == g.nb[a] ? 1u : 0u);     // points whose edges it owns: the last block also owns the boundary layer
        }
        for (uint32_t p = tid; p < kBlockPts; p += kSurfThreads) {
            const uint32_t lx = p % kP, ly = (p / kP) % kP, lz = p / (kP * kP);
            double v = 0.0;
            if (lx <= cnt[0] && ly <= cnt[1] && lz <= cnt[2]) {
                const double x = g.lo[0] + (double)(base[0] + lx) * g.h[0], y = g.lo[1] + (double)(base[1] + ly) * g.h[1],
                             z = g.lo[2] + (double)(base[2] + lz) * g.h[2];
                v = queryPoint<MAXP>(t, x, y, z, sNl, sRec);
            }
            sV[p] = v;
            sIn[p] = v < iso ? 1 : 0;
        }
        __syncthreads();
        // slot e < 3 * 729: point e / 3, axis e % 3.  The block owns the edge if it owns its lower point; the edge exists if it stays in the lattice.
        auto crosses = [&](uint32_t e, uint32_t& p, uint32_t& ax) -> bool {
            p = e / 3u, ax = e - 3u * p;
            if (p >= kBlockPts) return false;
            const uint32_t l[3] = {p % kP, (p / kP) % kP, p / (kP * kP)};
            if (!(l[0] < own[0] && l[1] < own[1] && l[2] < own[2] && l[ax] < cnt[ax])) return false;
            const uint32_t s = ax == 0 ? 1u : (ax == 1 ? kP : kP * kP);
            return sIn[p] != sIn[p + s];
        };
        auto cubeCase = [&](uint32_t c, uint32_t (&l)[3]) -> uint64_t {  // packed case of cube slot c, 0 outside the block
            l[0] = c % kB, l[1] = (c / kB) % kB, l[2] = c / (kB * kB);
            if (!(l[0] < cnt[0] && l[1] < cnt[1] && l[2] < cnt[2])) return 0;
            const uint32_t p = l[0] + kP * (l[1] + kP * l[2]);
            uint32_t cs = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) cs |= (uint32_t)sIn[p + (k & 1u) + kP * ((k >> 1) & 1u) + kP * kP * (k >> 2)] << k;
            return sCase[cs];
        };
        uint32_t vw = 0;
        for (uint32_t r = 0; r < kEdgeRounds; ++r) {
            uint32_t p, ax;
            vw += (uint32_t)__popcll(__ballot(crosses(r * kSurfThreads + tid, p, ax)));
        }
        uint32_t tn[kCubeRounds];
        uint64_t pk[kCubeRounds];
        uint32_t cl[kCubeRounds][3];
        for (uint32_t r = 0; r < kCubeRounds; ++r) {
            pk[r] = cubeCase(r * kSurfThreads + tid, cl[r]);
            tn[r] = (uint32_t)(pk[r] & 7u);
            uint32_t sum = tn[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            if (lane == 0) sTW[r][wave] = sum;
        }
        if (lane == 0) sVW[wave] = vw;
        __syncthreads();
        if constexpr (!EMIT) {
            if (tid == 0) {
                o.vcount[ab] = sVW[0] + sVW[1] + sVW[2] + sVW[3];
                uint32_t ts = 0;
                for (uint32_t r = 0; r < kCubeRounds; ++r) ts += sTW[r][0] + sTW[r][1] + sTW[r][2] + sTW[r][3];
                o.tcount[ab] = ts;
            }
        } else {
            uint64_t vpos = o.vprefix[ab];
            for (uint32_t w = 0; w < wave; ++w) vpos += sVW[w];
            for (uint32_t r = 0; r < kEdgeRounds; ++r) {
                uint32_t p, ax;
                const bool c = crosses(r * kSurfThreads + tid, p, ax);
                const uint64_t m = __ballot(c);
                if (c) {
                    const uint64_t at = vpos + rankBelow(m);
                    const uint32_t l[3] = {p % kP, (p / kP) % kP, p / (kP * kP)};
                    const uint32_t idx[3] = {base[0] + l[0], base[1] + l[1], base[2] + l[2]};
                    const uint32_t s = ax == 0 ? 1u : (ax == 1 ? kP : kP * kP);
                    const double va = sV[p], vb = sV[p + s];
                    double q[3];
                    edgeVertex(g.lo, g.h, idx, ax, va, vb, iso, q);
                    o.vkey[at] = 3u * (idx[0] + g.np[0] * (idx[1] + g.np[1] * (uint64_t)idx[2])) + ax;
                    o.vidx[at] = at;
                    o.vxyz[3 * at] = q[0], o.vxyz[3 * at + 1] = q[1], o.vxyz[3 * at + 2] = q[2];
                }
                vpos += (uint64_t)__popcll(m);
            }
            uint64_t tpos = o.tprefix[ab];
            for (uint32_t r = 0; r < kCubeRounds; ++r) {
                uint64_t at = tpos + sumBelow(tn[r], lane);
                for (uint32_t w = 0; w < wave; ++w) at += sTW[r][w];
                if (tn[r] != 0) {
                    const uint32_t i = base[0] + cl[r][0], j = base[1] + cl[r][1], k = base[2] + cl[r][2];
                    const uint64_t Q = i + g.n[0] * (j + g.n[1] * (uint64_t)k);
                    for (uint32_t tr = 0; tr < tn[r]; ++tr) {
                        o.tkey[at + tr] = 8u * Q + tr;
                        o.tidx[at + tr] = at + tr;
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            const uint32_t cr = caseCorner(pk[r], tr, m);
                            const uint64_t L = (i + (cr & 1u)) + g.np[0] * ((j + ((cr >> 1) & 1u)) + g.np[1] * (uint64_t)(k + (cr >> 2)));
                            o.tedge[3 * (at + tr) + m] = 3u * L + caseAxis(pk[r], tr, m);
                        }
                    }
                }
                tpos += sTW[r][0] + sTW[r][1] + sTW[r][2] + sTW[r][3];
            }
        }
    }
}

__global__ __launch_bounds__(kSurfThreads) void sparse_gather_kernel(const uint64_t* __restrict__ order, const double* __restrict__ xyz, uint64_t n,
                                                                 double* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t s = order[i];
        out[3 * i] = xyz[3 * s], out[3 * i + 1] = xyz[3 * s + 1], out[3 * i + 2] = xyz[3 * s + 2];
    }
}

// triangle i of the sorted order: its three edge ids -> their ranks among the sorted vertex keys (every one of them is there)
__global__ __launch_bounds__(kSurfThreads) void sparse_renumber_kernel(const uint64_t* __restrict__ order, const uint64_t* __restrict__ tedge, uint64_t nTris,
                                                                   const uint64_t* __restrict__ vkeys, uint64_t nVerts, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSurfThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kSurfThreads + threadIdx.x; i < nTris; i += stride) {
        const uint64_t s = order[i];
        for (int m = 0; m < 3; ++m) {
            const uint64_t e = tedge[3 * s + m];
            uint64_t lo = 0, hi = nVerts;  // first position whose key is >= e
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (vkeys[mid] < e)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            out[3 * i + m] = lo;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

struct IsActive {
    __host__ __device__ uint64_t operator()(uint8_t c) const { return c == 0 ? 1u : 0u; }
};
struct IsActiveFlag {
    __host__ __device__ bool operator()(uint8_t c) const { return c == 0; }
};

// the arguments of the three entry points -> the lattice; what: the entry point's name for the messages
int makeLattice(const char* what, const double* rc, const double* ris, const double* lo, const double* hi, const uint32_t* n, double iso,
                SparseLattice* out, CheckedLattice* checked = nullptr) {
    CheckedLattice cl{};
    if (const int r = checkLattice(what, kSparseLimits, rc, ris, lo, hi, n, iso, &cl)) return r;
    SparseLattice g{};
    g.nBlocks = 1;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = cl.lo[a], g.h[a] = cl.h[a], g.n[a] = cl.n[a];
        g.np[a] = (uint64_t)cl.n[a] + 1u;
        g.nb[a] = (cl.n[a] + kB - 1) / kB;
        g.nBlocks *= g.nb[a];
    }
    *out = g;
    if (checked) *checked = cl;
    return HPSDF_OK;
}

unsigned bitsFor(uint64_t maxKey) {  // radix passes stop at the highest bit a key can have
    unsigned b = 1;
    while (b < 64 && (maxKey >> b) != 0) ++b;
    return b;
}

// constants of the tree's leaves and the classes of blocks [first, first + count) into dClass; the stream is not synchronised
int classifyOnDevice(hpsdf_ctx* ctx, const hpsdf_tree* t, DevPool& pool, const SparseLattice& g, double iso, uint64_t first,
                     uint64_t count, uint8_t* dClass, unsigned long long* dVisited) {
    hipStream_t s = ctx->stream;
    const uint32_t nNodes = (uint32_t)t->nNodes;
    uint8_t* dDepth = nullptr;
    double* dConsts = nullptr;
    SURF_ALLOC(pool, dDepth, (size_t)nNodes, "node depths");
    SURF_ALLOC(pool, dConsts, (size_t)nNodes * 4 * sizeof(double), "leaf constants");
    HPSDF_HIP(launchLeafConsts(s, t, ctx->dTables, dDepth, dConsts));
    ClsTree ct{};
    ct.nodes = t->dev.nodes, ct.coeffs = t->dev.coeffs, ct.consts = dConsts;
    for (int a = 0; a < 3; ++a) ct.rootCentre[a] = t->dev.rootCentre[a], ct.rootInvSizes[a] = t->dev.rootInvSizes[a];
    hipLaunchKernelGGL(sparse_classify_kernel, dim3(gridOf(count)), dim3(kSurfThreads), 0, s, ct, ctx->dTables, g, iso, first, count, dClass, dVisited);
    HPSDF_HIP(hipGetLastError());
    return HPSDF_OK;
}

template <bool EMIT>
hipError_t launchBlocks(hipStream_t s, const TreeDev& td, const DeviceTables* T, const SparseLattice& g, double iso, const uint64_t* dActive,
                        uint64_t nActive, const BlockOut& o) {
    const dim3 grid((unsigned)(nActive < (1u << 20) ? nActive : (1u << 20))), block(kSurfThreads);
    forMaxDegree<3, 5, 12>(td.maxDegree, [&](auto P) {
        hipLaunchKernelGGL((sparse_block_kernel<decltype(P)::value, EMIT>), grid, block, 0, s, td, T, g, iso, dActive, nActive, o);
    });
    return hipGetLastError();
}

int extractSparse(hpsdf_ctx* ctx, const hpsdf_tree* t, const double* lo, const double* hi, const uint32_t* n, double iso, double** verts,
                  uint64_t* nVerts, uint64_t** tris, uint64_t* nTris, hpsdf_surface_sparse_stats* stats) {
    static const char* kWhat = "hpsdf_extract_surface_sparse";
    SparseLattice g{};
    CheckedLattice cl{};
    if (const int rc = makeLattice(kWhat, t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, iso, &g, &cl)) return rc;
    HPSDF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevPool pool(kWhat);
    Events<9> ev;
    TreeDev td = t->dev;
    td.leftAssoc = reductionLeftAssoc(ctx);
    hpsdf_surface_sparse_stats st{};
    st.blocks = g.nBlocks;

    // classes
    uint8_t* dClass = nullptr;
    unsigned long long* dScalars = nullptr;  // [0] visited leaves, [1] active blocks, [2] selected count
    SURF_ALLOC(pool, dClass, (size_t)g.nBlocks, "block classes");
    SURF_ALLOC(pool, dScalars, 3 * sizeof(unsigned long long), "counters");
    ev.mark(0, s);
    HPSDF_HIP(hipMemsetAsync(dScalars, 0, 3 * sizeof(unsigned long long), s));
    if (const int rc = classifyOnDevice(ctx, t, pool, g, iso, 0, g.nBlocks, dClass, dScalars)) return rc;
    ev.mark(1, s);

    // the active blocks, in block order
    using ActiveCount = rocprim::transform_iterator<const uint8_t*, IsActive, uint64_t>;
    using ActiveFlag = rocprim::transform_iterator<const uint8_t*, IsActiveFlag, bool>;
    size_t tmpBytes = 0;
    void* dTmp = nullptr;
    if (const int rc = withTemp(pool, "rocprim::reduce", "reduce storage", dTmp, tmpBytes, [&](void* tmp, size_t& bytes) {
            return rocprim::reduce(tmp, bytes, ActiveCount(dClass, IsActive()), (uint64_t*)(dScalars + 1), (uint64_t)0, (size_t)g.nBlocks,
                                   rocprim::plus<uint64_t>(), s);
        }))
        return rc;
    unsigned long long scal[2] = {0, 0};
    HPSDF_HIP(hipMemcpyAsync(scal, dScalars, sizeof scal, hipMemcpyDeviceToHost, s));
    HPSDF_HIP(hipStreamSynchronize(s));
    pool.release(dTmp);
    st.leaves_visited = scal[0];
    st.active_blocks = scal[1];
    const uint64_t nActive = scal[1];

    uint64_t V = 0, T = 0;
    uint64_t *dActive = nullptr, *dVp = nullptr, *dTp = nullptr;
    if (nActive > 0) {
        SURF_ALLOC(pool, dActive, nActive * 8, "active blocks");
        if (const int rc = withTemp(pool, "rocprim::select", "select storage", dTmp, tmpBytes, [&](void* tmp, size_t& bytes) {
                return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint64_t>(0), ActiveFlag(dClass, IsActiveFlag()), dActive,
                                       (uint64_t*)(dScalars + 2), (size_t)g.nBlocks, s);
            }))
            return rc;
        ev.mark(2, s);
        // per-block counts and their prefixes
        uint32_t *dVc = nullptr, *dTc = nullptr;
        SURF_ALLOC(pool, dVc, (nActive + 1) * 4, "vertex counts");
        SURF_ALLOC(pool, dTc, (nActive + 1) * 4, "triangle counts");
        SURF_ALLOC(pool, dVp, (nActive + 1) * 8, "vertex prefixes");
        SURF_ALLOC(pool, dTp, (nActive + 1) * 8, "triangle prefixes");
        HPSDF_HIP(hipMemsetAsync(dVc + nActive, 0, 4, s));
        HPSDF_HIP(hipMemsetAsync(dTc + nActive, 0, 4, s));
        BlockOut o{};
        o.vcount = dVc, o.tcount = dTc;
        HPSDF_HIP(launchBlocks<false>(s, td, ctx->dTables, g, iso, dActive, nActive, o));
        ev.mark(3, s);
        HPSDF_HIP(hipStreamSynchronize(s));  // (select's storage is free again)
        pool.release(dTmp);
        pool.release(dClass);
        if (const int rc = withTemp(pool, kPrefixScan, "scan storage", dTmp, tmpBytes, prefixScan(dVc, dVp, nActive + 1, s))) return rc;
        if (const int rc = primStatus(prefixScan(dTc, dTp, nActive + 1, s)(dTmp, tmpBytes), kPrefixScan)) return rc;  // (the same size: the same storage)
        ev.mark(4, s);
        HPSDF_HIP(hipMemcpyAsync(&V, dVp + nActive, 8, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(&T, dTp + nActive, 8, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(dTmp);
        pool.release(dVc);
        pool.release(dTc);
        st.classify_ms = ev.ms(0, 1), st.scan_ms = ev.ms(1, 2) + ev.ms(3, 4), st.count_ms = ev.ms(2, 3);
    } else {
        st.classify_ms = ev.ms(0, 1);
    }

    MeshOut mesh;
    if (T > 0) {
        if (const int rc = mesh.alloc(kWhat, V, T)) return rc;
        // records
        BlockOut o{};
        o.vprefix = dVp, o.tprefix = dTp;
        SURF_ALLOC(pool, o.vkey, V * 8, "vertex keys");
        SURF_ALLOC(pool, o.vidx, V * 8, "vertex indices");
        SURF_ALLOC(pool, o.vxyz, V * 24, "vertex records");
        SURF_ALLOC(pool, o.tkey, T * 8, "triangle keys");
        SURF_ALLOC(pool, o.tidx, T * 8, "triangle indices");
        SURF_ALLOC(pool, o.tedge, T * 24, "triangle records");
        ev.mark(5, s);
        HPSDF_HIP(launchBlocks<true>(s, td, ctx->dTables, g, iso, dActive, nActive, o));
        ev.mark(6, s);
        // vertices in edge-id order
        uint64_t *dVkS = nullptr, *dViS = nullptr, *dTkS = nullptr, *dTiS = nullptr;
        double* dVerts = nullptr;
        uint64_t* dTris = nullptr;
        const unsigned vBits = bitsFor(3 * cl.nPts), tBits = bitsFor(8 * cl.nCubes);
        SURF_ALLOC(pool, dVkS, V * 8, "sorted vertex keys");
        SURF_ALLOC(pool, dViS, V * 8, "sorted vertex indices");
        if (const int rc = withTemp(pool, "rocprim::radix_sort_pairs", "sort storage", dTmp, tmpBytes, [&](void* tmp, size_t& bytes) {
                return rocprim::radix_sort_pairs(tmp, bytes, o.vkey, dVkS, o.vidx, dViS, (size_t)V, 0u, vBits, s);
            }))
            return rc;
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(dTmp);
        pool.release(o.vkey);
        pool.release(o.vidx);
        pool.release(dActive);
        pool.release(dVp);
        pool.release(dTp);
        SURF_ALLOC(pool, dVerts, V * 24, "vertices");
        hipLaunchKernelGGL(sparse_gather_kernel, dim3(gridOf(V)), dim3(kSurfThreads), 0, s, dViS, o.vxyz, V, dVerts);
        HPSDF_HIP(hipGetLastError());
        // triangles in key order, renumbered
        SURF_ALLOC(pool, dTkS, T * 8, "sorted triangle keys");
        SURF_ALLOC(pool, dTiS, T * 8, "sorted triangle indices");
        if (const int rc = withTemp(pool, "rocprim::radix_sort_pairs", "sort storage", dTmp, tmpBytes, [&](void* tmp, size_t& bytes) {
                return rocprim::radix_sort_pairs(tmp, bytes, o.tkey, dTkS, o.tidx, dTiS, (size_t)T, 0u, tBits, s);
            }))
            return rc;
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(dTmp);
        pool.release(o.tkey);
        pool.release(o.tidx);
        pool.release(dTkS);
        pool.release(o.vxyz);
        pool.release(dViS);
        SURF_ALLOC(pool, dTris, T * 24, "triangles");
        hipLaunchKernelGGL(sparse_renumber_kernel, dim3(gridOf(T)), dim3(kSurfThreads), 0, s, dTiS, o.tedge, T, dVkS, V, dTris);
        HPSDF_HIP(hipGetLastError());
        ev.mark(7, s);
        if (const int rc = mesh.download(dVerts, dTris, s)) return rc;
        ev.mark(8, s);
        HPSDF_HIP(hipStreamSynchronize(s));
        st.emit_ms = ev.ms(5, 6), st.sort_ms = ev.ms(6, 7), st.download_ms = ev.ms(7, 8), st.total_ms = ev.ms(0, 8);
        mesh.handOver(verts, nVerts, tris, nTris);
    } else {
        ev.mark(8, s);
        HPSDF_HIP(hipStreamSynchronize(s));
        st.total_ms = ev.ms(0, 8);
    }
    st.peak_scratch_bytes = pool.peak;
    if (stats) *stats = st;
    return HPSDF_OK;
}

}  // namespace

}  // namespace hpsdf

using namespace hpsdf;

extern "C" {

int hpsdf_extract_surface_sparse(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3], double iso,
                                 double** verts, uint64_t* nVerts, uint64_t** tris, uint64_t* nTris, hpsdf_surface_sparse_stats* stats) {
    HPSDF_TRY
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || !lo || !hi || !n || !verts || !nVerts || !tris || !nTris) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    *verts = nullptr, *tris = nullptr, *nVerts = 0, *nTris = 0;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    return extractSparse(ctx, t, lo, hi, n, iso, verts, nVerts, tris, nTris, stats);
    HPSDF_CATCH
}

int hpsdf_surface_classify_host(const void* block, size_t size, const double lo[3], const double hi[3], const uint32_t n[3], double iso,
                                uint64_t first_block, uint64_t count, uint8_t* out) {
    HPSDF_TRY
    static const char* kWhat = "hpsdf_surface_classify_host";
    if (!lo || !hi || !n || (!out && count)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    HostTree ht;
    if (const int rc = parseBlock(block, size, &ht)) return rc;
    SparseLattice g{};
    if (const int rc = makeLattice(kWhat, ht.view.rootCentre, ht.view.rootInvSizes, lo, hi, n, iso, &g)) return rc;
    if (first_block > g.nBlocks || count > g.nBlocks - first_block)
        return fail(HPSDF_ERR_INVALID_ARGUMENT, std::string(kWhat) + ": the block range ends past the lattice's blocks");
    const HostEval eval{&tables()};
    for (uint64_t i = 0; i < count; ++i) {
        uint32_t visited;
        out[i] = classifyBlock(ht.view, g, iso, first_block + i, eval, visited);
    }
    return HPSDF_OK;
    HPSDF_CATCH
}

int hpsdf_surface_classify_device(hpsdf_ctx* ctx, const hpsdf_tree* t, const double lo[3], const double hi[3], const uint32_t n[3], double iso,
                                  uint64_t first_block, uint64_t count, uint8_t* out) {
    HPSDF_TRY
    static const char* kWhat = "hpsdf_surface_classify_device";
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!t || !lo || !hi || !n || (!out && count)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->device != ctx->device) return fail(HPSDF_ERR_INVALID_ARGUMENT, "tree lives on another device");
    SparseLattice g{};
    if (const int rc = makeLattice(kWhat, t->dev.rootCentre, t->dev.rootInvSizes, lo, hi, n, iso, &g)) return rc;
    if (first_block > g.nBlocks || count > g.nBlocks - first_block)
        return fail(HPSDF_ERR_INVALID_ARGUMENT, std::string(kWhat) + ": the block range ends past the lattice's blocks");
    if (count == 0) return HPSDF_OK;
    HPSDF_HIP(hipSetDevice(ctx->device));
    DevPool pool(kWhat);
    uint8_t* dClass = nullptr;
    SURF_ALLOC(pool, dClass, (size_t)count, "block classes");
    if (const int rc = classifyOnDevice(ctx, t, pool, g, iso, first_block, count, dClass, nullptr)) return rc;
    HPSDF_HIP(hipMemcpyAsync(out, dClass, (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    HPSDF_HIP(hipStreamSynchronize(ctx->stream));
    return HPSDF_OK;
    HPSDF_CATCH
}

}  // extern "C"
