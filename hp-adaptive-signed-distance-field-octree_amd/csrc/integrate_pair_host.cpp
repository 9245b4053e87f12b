// IntegratePair (include/hpsdf.h) on the calling thread: Integrate's host lists (integrate.hpp) with integrate_pair.hpp's cell statements
// and Query's leaf evaluation -- the statements of the kernels of integrate_pair.hip, the rows reduced by the same rule -- and the
// device-free entry.  Needs host_query.cpp (integrateArgumentError) and tables.cpp, and nothing of the device.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "integrate.hpp"
#include "integrate_pair.hpp"
#include "runtime.hpp"
#include "tables.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

struct HostPairCells {
    const ClsTree& tA;
    const ClsTree& tB;
    const PairArgs& p;
    uint32_t samples;
    HostEval eval;
    HostBoundsStack st;
    uint32_t cls(const IntegrateCell& c, int level, bool* finite) { return pairCellClass(tA, tB, p, c, level, eval, st, finite); }
    void row(const IntegrateCell& c, int level, double (&row)[kIntRow]) { pairCellRow(tA, tB, p, c, level, samples, eval, row); }
};

}  // namespace

int hostIntegratePair(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const PairArgs& p, const IntegrateArgs& a, hpsdf_integral* out,
                      hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    HostPairCells cells{tA, tB, p, a.samples, HostEval{&tables()}, {}};
    return hostIntegrateLists(cells, tA, nNodesA, a, out, outCells, outCount);
}

// what hpsdf_integrate_pair_* reject before anything runs (0: fine)
int pairArgumentError(uint32_t op, const double* pose, double isoA, double isoB, uint32_t depth, uint32_t samples, uint32_t maxCells,
                      uint32_t maxLeaves, const void* out, const void* outCells, const void* outCount) {
    if (!pose) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    if (op > HPSDF_PAIR_DIFFERENCE) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: op must be HPSDF_PAIR_INTERSECTION, _UNION or _DIFFERENCE");
    for (int k = 0; k < 12; ++k)
        if (!(std::fabs(pose[k]) <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: every entry of the pose must be finite");
    if (!(std::fabs(isoB) <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: iso_b must be finite");
    if (maxLeaves < 1u || maxLeaves > 65535u) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_integrate_pair: max_leaves must be in 1..65535");
    return integrateArgumentError(isoA, depth, samples, maxCells, out, outCells, outCount);
}

}  // namespace hpsdf

// IntegratePair from two serialised blocks, on the calling thread (no device): list 0 from A's records, both trees' constants from
// leafBound on the host
extern "C" int hpsdf_integrate_pair_block(const void* block_a, size_t size_a, const void* block_b, size_t size_b, uint32_t op, const double pose[12],
                                          double iso_a, double iso_b, uint32_t depth, uint32_t samples, uint32_t max_cells, uint32_t max_leaves,
                                          hpsdf_integral* out, hpsdf_integrate_cell** out_cells, uint64_t* out_n_cells) {
    using namespace hpsdf;
    HPSDF_TRY
    if (const int rc = pairArgumentError(op, pose, iso_a, iso_b, depth, samples, max_cells, max_leaves, out, out_cells, out_n_cells)) return rc;
    HostTree hA, hB;
    if (const int rc = parseBlock(block_a, size_a, &hA)) return rc;
    if (const int rc = parseBlock(block_b, size_b, &hB)) return rc;
    const PairArgs p = pairArgs(hA.view, op, pose, iso_a, iso_b, max_leaves);
    const IntegrateArgs a{iso_a, depth, samples, max_cells};
    return hostIntegratePair(hA.view, hA.m.recs.size(), hB.view, p, a, out, out_cells, out_n_cells);
    HPSDF_CATCH
}
