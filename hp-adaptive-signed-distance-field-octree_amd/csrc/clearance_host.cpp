// Clearance (include/hpsdf.h) on the calling thread: clearance.hpp's level loop over host lists with Query's leaf evaluation -- the
// statements of the kernels of clearance.hip -- and the device-free entry.  Needs host_query.cpp and tables.cpp, and nothing of the device.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "clearance.hpp"
#include "integrate.hpp"
#include "integrate_pair.hpp"
#include "runtime.hpp"
#include "tables.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

struct HostClearanceLists {
    const ClsTree& tA;
    const ClsTree& tB;
    const PairArgs& p;
    uint32_t maxDepth;
    HostEval eval;
    HostBoundsStack st;
    std::vector<IntegrateCell> cur, next;
    std::vector<double> blo;
    std::vector<uint8_t> kind;

    int level(int level, uint32_t n, ClearanceLevel* v) {
        blo.assign(n, 0.0);
        kind.assign(n, 0);
        ClearanceCandidate cand{boundsInf(), 0.0, kClearanceNoPos};
        for (uint32_t i = 0; i < n; ++i) {
            bool ok = true;
            ClearanceCell o;
            clearanceCell(tA, tB, p, cur[i], level, eval, st, &ok, o);
            if (!ok) v->finite = false;
            cur[i].cls = (uint8_t)o.clsA;
            blo[i] = o.blo;
            if (clearanceBefore(o.vb, i, cand.vb, cand.pos)) cand = ClearanceCandidate{o.vb, o.va, i};
        }
        if (!v->finite) return HPSDF_OK;
        if (cand.vb < v->best) v->best = cand.vb, v->bestVa = cand.va, v->bestCell = cur[cand.pos], v->hasWitness = 1u;
        v->minFinal = v->minSplit = boundsInf();
        v->nOutside = v->nPruned = v->nSplit = v->nFinal = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = clearanceKind(cur[i].cls, blo[i], v->best, cur[i].depth, maxDepth);
            kind[i] = (uint8_t)k;
            if (k == kClearOutside) v->nOutside += 1;
            if (k == kClearPruned) v->nPruned += 1;
            if (k == kClearSplit) {
                v->nSplit += 1;
                if (blo[i] < v->minSplit) v->minSplit = blo[i];
            }
            if (k == kClearFinal) {
                v->nFinal += 1;
                if (blo[i] < v->minFinal) v->minFinal = blo[i];
            }
        }
        return HPSDF_OK;
    }

    int emit(int, uint32_t n, bool split, uint32_t nSplit, uint32_t, std::vector<IntegrateCell>* cells, std::vector<double>& finalBlo) {
        next.clear();
        if (split) next.reserve(8 * (size_t)nSplit);
        for (uint32_t i = 0; i < n; ++i) {
            const IntegrateCell& c = cur[i];
            if (kind[i] == kClearSplit && split) {
                for (uint32_t ch = 0; ch < 8u; ++ch) next.push_back(integrateChild(c, ch));
            } else if (kind[i] == kClearSplit || kind[i] == kClearFinal) {
                if (cells) cells->push_back(c);
                finalBlo.push_back(blo[i]);
            }
        }
        cur.swap(next);
        return HPSDF_OK;
    }
};

}  // namespace

int hostClearance(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const PairArgs& p, const ClearanceArgs& a, hpsdf_clearance* out,
                  hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HostClearanceLists L{tA, tB, p, a.depth, HostEval{&tables()}, {}, {}, {}, {}, {}};
    integrateLeafCells(tA.nodes, nNodesA, L.cur);
    ClearanceSums S;
    if (const int rc = clearanceLevels(L, tA, p, a, (uint32_t)L.cur.size(), outCells != nullptr, S)) return rc;
    return clearanceHandOver(S, out, outCells, outCount);
}

// what hpsdf_clearance_* reject before anything runs (0: fine)
int clearanceArgumentError(const double* pose, double isoA, uint32_t depth, double tol, uint32_t maxCells, uint32_t maxLeaves, const void* out,
                           const void* outCells, const void* outCount) {
    if (!pose) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < 12; ++k)
        if (!(std::fabs(pose[k]) <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: every entry of the pose must be finite");
    if (!(std::fabs(isoA) <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: iso_a must be finite");
    if (!(tol >= 0.0 && tol <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: tol must be finite and >= 0");
    if (depth > 15u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: depth must be in 0..15");
    if (maxCells < 8u || maxCells > (1u << 28)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: max_cells must be in 8..2^28");
    if (maxLeaves < 1u || maxLeaves > 65535u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance: max_leaves must be in 1..65535");
    if (!out || (outCells != nullptr) != (outCount != nullptr)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    return HPSDF_OK;
}

// what hpsdf_clearance_batch_* reject before anything runs (0: fine).  n == 0 is the caller's to answer first.
int clearanceBatchArgumentError(const double* poses, size_t n, double isoA, uint32_t depth, double tol, double decide, uint32_t maxCells,
                                uint32_t maxLeaves, uint32_t maxTotalCells, const void* out) {
    if (n > ((size_t)1 << 24)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: n must be at most 2^24");
    if (!poses) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = clearanceArgumentError(poses, isoA, depth, tol, maxCells, maxLeaves, out, nullptr, nullptr)) return rc;
    if (!(decide != decide || std::fabs(decide) <= DBL_MAX))
        return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: decide must be finite or a NaN");
    if (maxTotalCells < maxCells || maxTotalCells > (1u << 28))
        return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: max_total_cells must be in max_cells..2^28");
    for (size_t i = 1; i < n; ++i)
        for (int k = 0; k < 12; ++k)
            if (!(std::fabs(poses[12 * i + k]) <= DBL_MAX))
                return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_clearance_batch: every entry of every pose must be finite");
    return HPSDF_OK;
}

int hostClearanceBatch(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const double* poses, size_t n, double isoA, uint32_t maxLeaves,
                       const ClearanceArgs& a, hpsdf_clearance* out) {
    std::vector<hpsdf_clearance> res(n);  // (a failure half way writes nothing)
    for (size_t i = 0; i < n; ++i) {
        const PairArgs p = pairArgs(tA, HPSDF_PAIR_INTERSECTION, poses + 12 * i, isoA, 0.0, maxLeaves);
        if (const int rc = hostClearance(tA, nNodesA, tB, p, a, &res[i], nullptr, nullptr)) return rc;
    }
    std::memcpy(out, res.data(), n * sizeof(hpsdf_clearance));
    return HPSDF_OK;
}

}  // namespace hpsdf

// ClearanceBatch from two serialised blocks, on the calling thread (no device): a loop of the single call with `decide`
extern "C" int hpsdf_clearance_batch_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, const double* poses, size_t n,
                                           double iso_a, uint32_t depth, double tol, double decide, uint32_t max_cells, uint32_t max_leaves,
                                           uint32_t max_total_cells, hpsdf_clearance* out) {
    using namespace hpsdf;
    HPSDF_TRY
    if (n == 0) return HPSDF_OK;
    if (const int rc = clearanceBatchArgumentError(poses, n, iso_a, depth, tol, decide, max_cells, max_leaves, max_total_cells, out)) return rc;
    HostTree hA, hB;
    if (const int rc = parseBlock(block_a, size_a, &hA)) return rc;
    if (const int rc = parseBlock(block_b, size_b, &hB)) return rc;
    const ClearanceArgs a{depth, max_cells, tol, decide};
    return hostClearanceBatch(hA.view, hA.m.recs.size(), hB.view, poses, n, iso_a, max_leaves, a, out);
    HPSDF_CATCH
}

// Clearance from two serialised blocks, on the calling thread (no device): list 0 from A's records, both trees' constants from leafBound
// on the host
extern "C" int hpsdf_clearance_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, const double pose[12], double iso_a,
                                     uint32_t depth, double tol, uint32_t max_cells, uint32_t max_leaves, hpsdf_clearance* out,
                                     hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = clearanceArgumentError(pose, iso_a, depth, tol, max_cells, max_leaves, out, out_cells, out_n_cells)) return rc;
    HostTree hA, hB;
    if (const int rc = parseBlock(block_a, size_a, &hA)) return rc;
    if (const int rc = parseBlock(block_b, size_b, &hB)) return rc;
    const PairArgs p = pairArgs(hA.view, HPSDF_PAIR_INTERSECTION, pose, iso_a, 0.0, max_leaves);
    const ClearanceArgs a{depth, max_cells, tol};
    return hostClearance(hA.view, hA.m.recs.size(), hB.view, p, a, out, out_cells, out_n_cells);
    HPSDF_CATCH
}
