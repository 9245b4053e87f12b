// Simplify on the device (include/hpsdf.h, "Simplify"; the statements are simplify.hpp's, the levels are driven from the host like
// Integrate's).
//
//   simplify_candidates_kernel      one lane per interior node of the level: eight leaf children?  then q = their largest degree; the
//                                   node's record for the scan: (1, 0, count[q]) for q <= kSimpLowQ, (0, 1, count[q]) above, zeros if not.
//   (rocprim::exclusive_scan)       the records -> each candidate's rank in its degree class and the offset of its rows in the arena.
//   simplify_list_kernel            one lane per interior node of the level: a candidate writes {node, q, rows offset} at its rank.
//   simplify_merge_kernel<Q, G>     the hot path.  A group of G lanes per candidate: one wave (G = 64, four candidates a workgroup) for
//                                   q <= 5, where the 56 entries of the largest polynomial are one per lane, and the whole workgroup
//                                   (G = 256) for q <= 12 (455 entries, two per lane).  Per group two cubes of Q^3 doubles in LDS (Q = 6:
//                                   3.4 KB a group; Q = 13: 34.3 KB), the parent's entries and the residual's partial sums; lanes own
//                                   entries, each a serial dot product of at most 13 terms in simplify.hpp's order.  T is lower
//                                   triangular and the basis has bounded total degree, so of a cube only the entries with
//                                   x + y + z <= q exist: 56 of 216, 455 of 2197 -- a pass is entries x (at most q + 1) multiply-adds,
//                                   not Q^4.  The squares are reduced by simpReduce's tree through LDS, lane 0 of the group forms b and
//                                   decides, and an accepted candidate's rows, e and degree are written.
//   simplify_truncate_kernel        once at the end, one lane per surviving leaf: simpTruncate.
//
// Memory: 24 bytes a node (SimpNode), 4 per interior node (the level lists), the arena = the source's coefficients followed by room for
// every row the merges can make (SimpState::extBound, found on the host from the source's degrees), 16 + 16 bytes per interior node of
// the largest level (records and ranks), 16 per candidate.  What bounds the merge kernel: LDS latency behind the serial dot products
// (each term is one LDS load and one dependent multiply-add) and, for the workgroup class, the 75 barriers of a candidate; HBM traffic
// is the children's rows once per direction.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "dev_pool.hpp"
#include "device_types.hpp"
#include "runtime.hpp"
#include "simplify.hpp"

namespace hpsdf {

namespace {

constexpr uint32_t kSimpLowQ = 5;     // up to this degree a candidate is one wave's
constexpr unsigned kSimpThreads = 256;

struct CandSum {
    uint32_t low, high;
    uint64_t rows;
};
struct CandPlus {
    __host__ __device__ CandSum operator()(const CandSum& a, const CandSum& b) const { return CandSum{a.low + b.low, a.high + b.high, a.rows + b.rows}; }
};
struct SimpCand {
    uint32_t node, q;
    uint64_t rowsAt;  // in the arena
};

// the largest child degree of `node` if its eight children are leaves, else 13
__device__ __forceinline__ uint32_t candidateDegree(const SimpNode* __restrict__ nodes, uint32_t node) {
    const uint32_t first = nodes[node].child;
    uint32_t q = 0;
    for (uint32_t c = 0; c < 8u; ++c) {
        const uint32_t d = nodes[first + c].degree;
        q = d > q ? d : q;
    }
    return q;
}

__global__ __launch_bounds__(kSimpThreads) void simplify_candidates_kernel(const SimpNode* __restrict__ nodes, const uint32_t* __restrict__ level, uint32_t n,
                                                                           const DeviceTables* __restrict__ T, CandSum* __restrict__ recs) {
    const uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = candidateDegree(nodes, level[i]);
    recs[i] = q > (uint32_t)kMaxDegree ? CandSum{0u, 0u, 0ull} : CandSum{q <= kSimpLowQ ? 1u : 0u, q <= kSimpLowQ ? 0u : 1u, (uint64_t)T->count[q]};
}

__global__ __launch_bounds__(kSimpThreads) void simplify_list_kernel(const SimpNode* __restrict__ nodes, const uint32_t* __restrict__ level, uint32_t n,
                                                                     const CandSum* __restrict__ ranks, uint64_t base, SimpCand* __restrict__ low,
                                                                     SimpCand* __restrict__ high) {
    const uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = level[i], q = candidateDegree(nodes, node);
    if (q > (uint32_t)kMaxDegree) return;
    const CandSum r = ranks[i];
    const SimpCand c{node, q, base + r.rows};
    if (q <= kSimpLowQ)
        low[r.low] = c;
    else
        high[r.high] = c;
}

// Q: entries per axis of the cubes (the class's largest degree + 1); G: lanes of a candidate's group.
template <int Q, int G>
__global__ __launch_bounds__(kSimpThreads) void simplify_merge_kernel(SimpNode* __restrict__ nodes, double* __restrict__ arena, const SimpCand* __restrict__ cands,
                                                                      uint32_t n, const DeviceTables* __restrict__ T, double rms) {
    constexpr int kGroups = kSimpThreads / G;
    constexpr int kEntries = Q * (Q + 1) * (Q + 2) / 6;  // simpEntries(Q - 1)
    constexpr int kP2 = kEntries <= 64 ? 64 : 512;       // >= simpPow2 of any entry count of the class
    using C = SimpCube<Q>;
    __shared__ double sT[2 * kSimpQ * kSimpQ];
    __shared__ double sU[kGroups][Q * Q * Q];
    __shared__ double sV[kGroups][Q * Q * Q];
    __shared__ double sP[kGroups][kEntries];
    __shared__ double sAcc[kGroups][kP2];
    __shared__ uint8_t sB[kEntries][4];
    __shared__ uint32_t sAccept[kGroups];
    for (int i = threadIdx.x; i < 2 * kSimpQ * kSimpQ; i += kSimpThreads) sT[i] = (&T->transfer[0][0][0])[i];
    for (int i = threadIdx.x; i < kEntries * 4; i += kSimpThreads) (&sB[0][0])[i] = (&T->bidx[0][0])[i];
    const uint32_t g = threadIdx.x / G, l = threadIdx.x % G;
    const uint32_t idx = blockIdx.x * kGroups + g;
    const bool active = idx < n;  // (an idle group still meets every barrier below)
    const SimpCand cd = active ? cands[idx] : SimpCand{0u, 0u, 0ull};
    const uint32_t q = cd.q < (uint32_t)Q ? cd.q : (uint32_t)(Q - 1);  // (a candidate of this class: q < Q)
    const uint32_t entries = active ? simpEntries(q) : 0u, p2 = simpPow2(entries);
    const uint32_t stored = active ? T->count[q] : 0u;
    const uint32_t first = active ? nodes[cd.node].child : 0u;
    double *U = sU[g], *V = sV[g], *P = sP[g], *acc = sAcc[g];
    for (uint32_t e = l; e < entries; e += G) P[e] = 0.0;
    __syncthreads();  // (the tables)
    for (uint32_t ch = 0; ch < 8u; ++ch) {
        const double* c = nullptr;
        uint32_t have = 0;
        if (active) {
            const SimpNode cn = nodes[first + ch];
            c = arena + cn.rowsAt;
            have = T->count[cn.degree <= kMaxDegree ? cn.degree : 0];
        }
        for (uint32_t e = l; e < entries; e += G) U[C::at(sB[e][0], sB[e][1], sB[e][2])] = e < have ? c[e] : 0.0;
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) V[C::at(sB[e][0], sB[e][1], sB[e][2])] = C::fwdX(sT, ch, U, sB[e][0], sB[e][1], sB[e][2]);
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) U[C::at(sB[e][0], sB[e][1], sB[e][2])] = C::fwdY(sT, ch, V, sB[e][0], sB[e][1], sB[e][2]);
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) P[e] = P[e] + C::fwdZ(sT, ch, U, sB[e][0], sB[e][1], sB[e][2]);
        __syncthreads();
    }
    for (uint32_t e = l; e < entries; e += G)
        if (e >= stored) P[e] = 0.0;  // (degree 6 stores 83 of its 84 entries; a lane's own entry)
    for (uint32_t t = l; t < p2; t += G) acc[t] = 0.0;
    double carried = 0.0;
    for (uint32_t ch = 0; ch < 8u; ++ch) {
        const double* c = nullptr;
        uint32_t have = 0;
        if (active) {
            const SimpNode cn = nodes[first + ch];
            c = arena + cn.rowsAt;
            have = T->count[cn.degree <= kMaxDegree ? cn.degree : 0];
            carried = carried + cn.e;
        }
        for (uint32_t e = l; e < entries; e += G) U[C::at(sB[e][0], sB[e][1], sB[e][2])] = P[e];
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) V[C::at(sB[e][0], sB[e][1], sB[e][2])] = C::bwdZ(sT, ch, U, (int)q, sB[e][0], sB[e][1], sB[e][2]);
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) U[C::at(sB[e][0], sB[e][1], sB[e][2])] = C::bwdY(sT, ch, V, (int)q, sB[e][0], sB[e][1], sB[e][2]);
        __syncthreads();
        for (uint32_t e = l; e < entries; e += G) {
            const double d = (e < have ? c[e] : 0.0) - C::bwdX(sT, ch, U, (int)q, sB[e][0], sB[e][1], sB[e][2]);
            acc[e] = acc[e] + d * d;
        }
        __syncthreads();
    }
    // simpReduce's steps, the group's lanes as t.  The trip count is the class's, not the candidate's, so that every group of the
    // workgroup meets the same barriers; a group whose p2 is smaller starts when the stride reaches its half.
    for (uint32_t stride = kP2 >> 1; stride > 0u; stride >>= 1) {
        if (stride < p2)
            for (uint32_t t = l; t < stride; t += G) acc[t] = acc[t] + acc[t + stride];
        __syncthreads();
    }
    if (l == 0u) {
        bool ok = false;
        if (active) {
            const double b = simpBound(acc[0], carried);
            ok = simpAccept(b, rms, nodes[cd.node].depth);
            if (ok) {
                nodes[cd.node].rowsAt = cd.rowsAt;
                nodes[cd.node].e = b;
                nodes[cd.node].degree = (uint8_t)q;
            }
        }
        sAccept[g] = ok ? 1u : 0u;
    }
    __syncthreads();
    if (sAccept[g] != 0u)
        for (uint32_t e = l; e < stored; e += G) arena[cd.rowsAt + e] = P[e];
}

__global__ __launch_bounds__(kSimpThreads) void simplify_truncate_kernel(SimpNode* __restrict__ nodes, const double* __restrict__ arena,
                                                                         const uint32_t* __restrict__ leaves, uint32_t n,
                                                                         const DeviceTables* __restrict__ T, double rms) {
    const uint32_t i = blockIdx.x * kSimpThreads + threadIdx.x;
    if (i >= n) return;
    SimpNode nd = nodes[leaves[i]];
    if (nd.degree > (uint8_t)kMaxDegree) return;
    double e = nd.e;
    const uint32_t d = simpTruncate(arena + nd.rowsAt, nd.degree, T->count, rms, nd.depth, &e);
    nodes[leaves[i]].degree = (uint8_t)d;
    nodes[leaves[i]].e = e;
}

inline uint32_t blocksOf(uint32_t n) { return (n + kSimpThreads - 1) / kSimpThreads; }

}  // namespace

// The passes over a state simplifyBegin made, on ctx's device: s.nodes and s.ext come back as simplifyOnHost leaves them.  Synchronises
// the context stream before it returns; frees everything it took, whatever happens.
int simplifyOnDevice(hpsdf_ctx* ctx, const BlockView& v, const BlockMirror& m, double rms, uint32_t flags, SimpState& s) {
    if (rms == 0.0) return HPSDF_OK;
    hipStream_t st = ctx->stream;
    DevPool pool{"hpsdf_simplify"};
    const size_t nn = s.nodes.size();
    const bool merge = (flags & HPSDF_SIMPLIFY_MERGE) != 0;
    const uint64_t arenaCount = v.nCoeffs + (merge ? s.extBound : 0);
    SimpNode* dNodes = nullptr;
    double* dArena = nullptr;
    SURF_ALLOC(pool, dNodes, nn * sizeof(SimpNode), "nodes");
    SURF_ALLOC(pool, dArena, (size_t)arenaCount * sizeof(double), "the arena");
    HPSDF_HIP(hipMemcpyAsync(dNodes, s.nodes.data(), nn * sizeof(SimpNode), hipMemcpyHostToDevice, st));
    if (v.nCoeffs) HPSDF_HIP(hipMemcpyAsync(dArena, v.coeffs, (size_t)v.nCoeffs * sizeof(double), hipMemcpyHostToDevice, st));
    const auto sync = [&]() { return hipStreamSynchronize(st); };
    struct Drain {  // (nothing of this call runs on when its arrays go)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    uint64_t used = 0;  // rows the levels so far took of the arena's second part (rejected candidates' included)
    if (merge) {
        size_t widest = 0;
        for (int D = m.walk.maxDepth; D >= 2; --D) widest = s.level[D - 1].size() > widest ? s.level[D - 1].size() : widest;
        uint32_t* dLevel = nullptr;
        CandSum *dRecs = nullptr, *dRanks = nullptr;
        SimpCand *dLow = nullptr, *dHigh = nullptr;
        if (widest != 0) {
            SURF_ALLOC(pool, dLevel, widest * sizeof(uint32_t), "a level's nodes");
            SURF_ALLOC(pool, dRecs, widest * sizeof(CandSum), "candidate records");
            SURF_ALLOC(pool, dRanks, widest * sizeof(CandSum), "candidate ranks");
            SURF_ALLOC(pool, dLow, widest * sizeof(SimpCand), "candidates");
            SURF_ALLOC(pool, dHigh, widest * sizeof(SimpCand), "candidates");
        }
        for (int D = m.walk.maxDepth; D >= 2; --D) {
            const std::vector<uint32_t>& lv = s.level[D - 1];
            const uint32_t n = (uint32_t)lv.size();
            if (n == 0) continue;
            HPSDF_HIP(hipMemcpyAsync(dLevel, lv.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(simplify_candidates_kernel, dim3(blocksOf(n)), dim3(kSimpThreads), 0, st, dNodes, dLevel, n, ctx->dTables, dRecs);
            HPSDF_HIP(hipGetLastError());
            void* tmp = nullptr;
            size_t bytes = 0;
            const CandSum* in = dRecs;
            CandSum* out = dRanks;
            if (const int rc = withTemp(pool, "rocprim::exclusive_scan", "scan storage", tmp, bytes, [=](void* p, size_t& b) {
                    return rocprim::exclusive_scan(p, b, in, out, CandSum{0u, 0u, 0ull}, (size_t)n, CandPlus(), st);
                }))
                return rc;
            CandSum last[2];
            HPSDF_HIP(hipMemcpyAsync(&last[0], dRanks + (n - 1), sizeof(CandSum), hipMemcpyDeviceToHost, st));
            HPSDF_HIP(hipMemcpyAsync(&last[1], dRecs + (n - 1), sizeof(CandSum), hipMemcpyDeviceToHost, st));
            HPSDF_HIP(sync());  // (lv stays alive until here: the level's upload has been read)
            pool.release(tmp);
            const uint32_t nLow = last[0].low + last[1].low, nHigh = last[0].high + last[1].high;
            const uint64_t rows = last[0].rows + last[1].rows;
            if (nLow + nHigh == 0) continue;
            if (used + rows > s.extBound) return fail(HPSDF_ERR_STATE, "hpsdf_simplify: the merges' rows outgrew their bound");
            s.levels += 1;
            hipLaunchKernelGGL(simplify_list_kernel, dim3(blocksOf(n)), dim3(kSimpThreads), 0, st, dNodes, dLevel, n, dRanks, v.nCoeffs + used, dLow, dHigh);
            HPSDF_HIP(hipGetLastError());
            if (nLow != 0) {
                hipLaunchKernelGGL((simplify_merge_kernel<kSimpLowQ + 1, 64>), dim3((nLow + 3) / 4), dim3(kSimpThreads), 0, st, dNodes, dArena, dLow, nLow,
                                   ctx->dTables, rms);
                HPSDF_HIP(hipGetLastError());
            }
            if (nHigh != 0) {
                hipLaunchKernelGGL((simplify_merge_kernel<kSimpQ, 256>), dim3(nHigh), dim3(kSimpThreads), 0, st, dNodes, dArena, dHigh, nHigh, ctx->dTables,
                                   rms);
                HPSDF_HIP(hipGetLastError());
            }
            used += rows;
        }
        HPSDF_HIP(hipMemcpyAsync(s.nodes.data(), dNodes, nn * sizeof(SimpNode), hipMemcpyDeviceToHost, st));
        HPSDF_HIP(sync());
        pool.release(dLevel), pool.release(dRecs), pool.release(dRanks), pool.release(dLow), pool.release(dHigh);
    }
    if (flags & HPSDF_SIMPLIFY_TRUNCATE) {
        std::vector<uint32_t> leaves;
        simplifyLeaves(s, leaves);
        const uint32_t n = (uint32_t)leaves.size();
        std::vector<uint8_t> before(n);
        for (uint32_t i = 0; i < n; ++i) before[i] = s.nodes[leaves[i]].degree;
        uint32_t* dLeaves = nullptr;
        SURF_ALLOC(pool, dLeaves, (size_t)n * sizeof(uint32_t), "the leaves");
        HPSDF_HIP(hipMemcpyAsync(dLeaves, leaves.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(simplify_truncate_kernel, dim3(blocksOf(n)), dim3(kSimpThreads), 0, st, dNodes, dArena, dLeaves, n, ctx->dTables, rms);
        HPSDF_HIP(hipGetLastError());
        HPSDF_HIP(hipMemcpyAsync(s.nodes.data(), dNodes, nn * sizeof(SimpNode), hipMemcpyDeviceToHost, st));
        HPSDF_HIP(sync());
        for (uint32_t i = 0; i < n; ++i) s.truncations += s.nodes[leaves[i]].degree != before[i] ? 1 : 0;
    }
    // The rows the merges made: the arena's second part as it is (a rejected candidate's slot is never read; the host path has no such
    // slots, but a block is made from the rows a node points at, not from where they lie).
    if (merge && used != 0) {
        s.ext.resize((size_t)used);
        HPSDF_HIP(hipMemcpyAsync(s.ext.data(), dArena + v.nCoeffs, (size_t)used * sizeof(double), hipMemcpyDeviceToHost, st));
        HPSDF_HIP(sync());
    }
    return HPSDF_OK;
}

}  // namespace hpsdf
