// Clearance (include/hpsdf.h, "Clearance"): the plain C++ part -- a cell's bound and witness value, the prune test, the level loop and
// the result.  Integrate's cells and lists (integrate.hpp), IntegratePair's pose, image box, clamp and point descent (integrate_pair.hpp)
// and QueryBounds' walk (tree_bound.hpp) are used as they are.  Shared by clearance.hip (the kernels), clearance_batch.hip (the
// kernels of many poses at once) and clearance_host.cpp (the same loop over host lists): one set of statements with a fixed association,
// built with -ffp-contract=off, so host and device give the same bits.  No HIP compiler is needed for this file.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "integrate.hpp"
#include "integrate_pair.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

struct ClearanceArgs {
    uint32_t depth, maxCells;
    double tol;
    double decide = boundsQuietNaN();  // the batch entries' decision threshold (a quiet NaN: off, the single call's rule)
};

// what a level's first kernel leaves of a cell: blo (step 1) and, for a candidate, vb and va (step 2; vb = +inf: no candidate)
struct ClearanceCell {
    double blo, vb, va;
    uint32_t clsA;
};

// a candidate of step 2: the lexicographic minimum of (vb, pos) is the level's
struct ClearanceCandidate {
    double vb, va;
    uint32_t pos;
};
constexpr uint32_t kClearanceNoPos = 0xFFFFFFFFu;

__host__ __device__ inline bool clearanceBefore(double vb, uint32_t pos, double wb, uint32_t qos) { return vb < wb || (vb == wb && pos < qos); }

// An order-preserving 64-bit key of a double that is not a NaN: clearanceKey(x) < clearanceKey(y) iff x < y, and equal keys iff x == y
// (-0.0 and +0.0 share a key, as they compare equal).  What the batch's integer atomicMin reduces (clearance_batch.hip); the least key
// of a pose and then the least pos among its holders is clearanceBefore's minimum.
__host__ __device__ inline uint64_t clearanceKey(double x) {
    if (x == 0.0) x = 0.0;  // -0.0 -> +0.0
    const uint64_t u = __builtin_bit_cast(unsigned long long, x);
    return (u >> 63) != 0u ? ~u : u | 0x8000000000000000ull;
}
constexpr uint64_t kClearanceNoKey = ~0ull;  // above every key of a double that is not a NaN: the start of a minimum
// the double of a key (+0.0 for either zero); kClearanceNoKey: +inf, an empty minimum
__host__ __device__ inline double clearanceKeyValue(uint64_t key) {
    if (key == kClearanceNoKey) return boundsInf();
    return __builtin_bit_cast(double, (unsigned long long)((key >> 63) != 0u ? key & 0x7FFFFFFFFFFFFFFFull : ~key));
}

// Steps 1 and 2 of a cell.  *finite: false if A's cell or a leaf of B's walk is not finite.
template <class Eval, class Stack>
__host__ __device__ inline void clearanceCell(const ClsTree& tA, const ClsTree& tB, const PairArgs& a, const IntegrateCell& c, int level,
                                              const Eval& eval, Stack& st, bool* finite, ClearanceCell& o) {
    const double inf = boundsInf();
    o.blo = inf, o.vb = inf, o.va = boundsQuietNaN();
    o.clsA = integrateCellClass(tA, c, level, a.isoA, eval, finite);
    if (!*finite || o.clsA == 1u) return;
    double lo[3], hi[3], pl[3], ph[3];
    bool partial;
    pairCellBox(tA, a, c, lo, hi);
    const uint32_t reach = pairClamp(tB, lo, hi, pl, ph, &partial);
    if (reach != 0u) {
        o.blo = reach == 1u ? inf : -inf;
        return;
    }
    BoundsRow R;
    boundsWalkRange(tB, pl, ph, 1u, a.maxLeaves, eval, st, R);
    if (R.status == HPSDF_BOUNDS_NOT_FINITE) *finite = false;
    o.blo = R.lo;
    double x[3], hx[3], y[3];
    pairCellCentre(tA, a, c, x, hx);
    const double va = pairQueryPoint(tA, x, eval);
    if (va < a.isoA) {
        pairImage(a, x, y);
        const double vb = pairQueryPoint(tB, y, eval);
        if (vb < DBL_MAX) o.vb = vb, o.va = va;
    }
}

// Step 3 of a cell: 0 dropped by A's class, 1 pruned, 2 a split candidate, 3 final
enum { kClearOutside = 0u, kClearPruned = 1u, kClearSplit = 2u, kClearFinal = 3u };
__host__ __device__ inline uint32_t clearanceKind(uint32_t clsA, double blo, double best, uint32_t cellDepth, uint32_t maxDepth) {
    if (clsA == 1u) return kClearOutside;
    if (!(blo <= best && blo < boundsInf())) return kClearPruned;
    return cellDepth < maxDepth ? kClearSplit : kClearFinal;
}

// What a level's steps leave (read back once a level on the device)
struct ClearanceLevel {
    double best = 0.0, bestVa = 0.0;           // after step 2
    IntegrateCell bestCell{};
    uint32_t hasWitness = 0;
    double minFinal = 0.0, minSplit = 0.0;     // the least blo of this level's finals and split candidates (+inf: none)
    uint64_t nOutside = 0, nPruned = 0, nSplit = 0, nFinal = 0;
    bool finite = true;
};

struct ClearanceSums {
    hpsdf_clearance r;
    std::vector<IntegrateCell> cells;  // the finals, when asked for
    std::vector<double> blo;           // their bounds
};

// the struct of a call that met a cell that is not finite
inline void clearanceNotFinite(uint32_t levels, hpsdf_clearance* r) {
    std::memset(r, 0, sizeof *r);
    const double nan = boundsQuietNaN();
    r->lo = -boundsInf(), r->hi = boundsInf(), r->value_a = nan;
    for (int k = 0; k < 3; ++k) r->point[k] = r->image[k] = nan;
    r->status = HPSDF_CLEARANCE_NOT_FINITE, r->levels = levels;
}

// The state of the level loop between two lists, and step 3's last lines on it (include/hpsdf.h, "Clearance", "The rule"): one set of
// statements for clearanceLevels and for the batch's decide kernel (clearance_batch.hip), a lane a pose.
struct ClearanceLoop {
    double finalsLo;           // the least blo of the finals so far (+inf: none)
    uint64_t nFinals;
    uint64_t visited, outside, pruned;
    uint32_t status, levels;
};
__host__ __device__ inline void clearanceLoopStart(ClearanceLoop& s) {
    s.finalsLo = boundsInf();
    s.nFinals = s.visited = s.outside = s.pruned = 0;
    s.status = HPSDF_CLEARANCE_EMPTY, s.levels = 0;
}
// the first lines of a level: its n cells were visited
__host__ __device__ inline void clearanceLoopVisit(ClearanceLoop& s, int level, uint32_t n) {
    s.visited += n;
    s.levels = (uint32_t)level;
}
enum { kClearLoopEmpty = 0, kClearLoopStop = 1, kClearLoopSplit = 2 };
// A finite level's counts and minima with the updated best -> kClearLoopEmpty: nothing is left and nothing was, the status stays EMPTY;
// kClearLoopStop: s.status says why, the split candidates join the finals; kClearLoopSplit: their children form the next list.
__host__ __device__ inline int clearanceLoopStep(ClearanceLoop& s, const ClearanceArgs& a, double best, double minFinal, double minSplit,
                                                 uint64_t nOutside, uint64_t nPruned, uint64_t nSplit, uint64_t nFinal) {
    s.outside += nOutside;
    s.pruned += nPruned;
    if (s.nFinals == 0 && nFinal == 0 && nSplit == 0) return kClearLoopEmpty;
    double Lmin = s.finalsLo;
    if (minFinal < Lmin) Lmin = minFinal;
    if (minSplit < Lmin) Lmin = minSplit;
    bool split = false;
    if (best - Lmin <= a.tol) s.status = HPSDF_CLEARANCE_CONVERGED;
    else if (Lmin > a.decide || best < a.decide) s.status = HPSDF_CLEARANCE_DECIDED;  // (both false when decide is a NaN)
    else if (8ull * nSplit > a.maxCells) s.status = HPSDF_CLEARANCE_CELL_LIMIT;
    else if (nSplit == 0) s.status = HPSDF_CLEARANCE_DEPTH;
    else split = true;
    s.nFinals += nFinal + (split ? 0u : nSplit);
    if (minFinal < s.finalsLo) s.finalsLo = minFinal;
    if (!split && minSplit < s.finalsLo) s.finalsLo = minSplit;
    return split ? kClearLoopSplit : kClearLoopStop;
}

// The struct of a call whose loop ended in s with a status other than NOT_FINITE; cells_open and the finals with blo > hi (which join
// cells_pruned) are the caller's to add.
inline void clearanceResult(const ClsTree& tA, const PairArgs& p, const ClearanceLoop& s, double best, double bestVa, const IntegrateCell& bestCell,
                            uint32_t hasWitness, hpsdf_clearance& r) {
    const double inf = boundsInf(), nan = boundsQuietNaN();
    std::memset(&r, 0, sizeof r);
    r.cells_visited = s.visited, r.cells_outside_a = s.outside, r.cells_pruned = s.pruned;
    r.levels = s.levels;
    r.status = s.status;
    r.value_a = nan;
    for (int k = 0; k < 3; ++k) r.point[k] = r.image[k] = nan;
    if (s.status == HPSDF_CLEARANCE_EMPTY) {
        r.lo = r.hi = inf;
        return;
    }
    r.hi = best;
    r.lo = s.finalsLo;
    if (hasWitness) {
        double x[3], hx[3], y[3];
        pairCellCentre(tA, p, bestCell, x, hx);
        pairImage(p, x, y);
        for (int k = 0; k < 3; ++k) r.point[k] = x[k], r.image[k] = y[k];
        r.value_a = bestVa;
    }
}

// The level loop and the result (include/hpsdf.h, "Clearance", "The rule").  Lists:
//   level(l, n, &v)                          steps 1 to 3 over the n cells of the current list: v
//   emit(l, n, split, nSplit, nFinal, cells, blo)   split: the split candidates' children become the current list and the nFinal finals
//                                            are appended to *cells (may be null) and blo; else all nSplit + nFinal survivors are
template <class Lists>
int clearanceLevels(Lists& L, const ClsTree& tA, const PairArgs& p, const ClearanceArgs& a, uint32_t n0, bool wantCells, ClearanceSums& S) {
    hpsdf_clearance& r = S.r;
    std::memset(&r, 0, sizeof r);
    ClearanceLevel v;
    v.best = boundsInf();
    ClearanceLoop s;
    clearanceLoopStart(s);
    uint32_t n = n0;
    for (int level = 0; n != 0; ++level) {
        if (const int rc = L.level(level, n, &v)) return rc;
        clearanceLoopVisit(s, level, n);
        if (!v.finite) {
            clearanceNotFinite(s.levels, &r);
            S.cells.clear(), S.blo.clear();
            return HPSDF_OK;
        }
        const int step = clearanceLoopStep(s, a, v.best, v.minFinal, v.minSplit, v.nOutside, v.nPruned, v.nSplit, v.nFinal);
        if (step == kClearLoopEmpty) break;
        const bool split = step == kClearLoopSplit;
        if (const int rc = L.emit(level, n, split, (uint32_t)v.nSplit, (uint32_t)v.nFinal, wantCells ? &S.cells : nullptr, S.blo)) return rc;
        if (!split) break;
        n = 8u * (uint32_t)v.nSplit;
    }
    clearanceResult(tA, p, s, v.best, v.bestVa, v.bestCell, v.hasWitness, r);
    if (s.status == HPSDF_CLEARANCE_EMPTY) {
        S.cells.clear(), S.blo.clear();
        return HPSDF_OK;
    }
    size_t kept = 0;
    for (size_t i = 0; i < S.blo.size(); ++i) {
        if (S.blo[i] > r.hi) {
            r.cells_pruned += 1;
            continue;
        }
        if (wantCells) S.cells[kept] = S.cells[i];
        S.blo[kept] = S.blo[i];
        ++kept;
    }
    S.blo.resize(kept);
    if (wantCells) S.cells.resize(kept);
    r.cells_open = kept;
    return HPSDF_OK;
}

// the struct and the optional malloc'd cell array into the caller's outputs (Integrate's convention: an empty result is NULL, 0)
inline int clearanceHandOver(const ClearanceSums& S, hpsdf_clearance* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    hpsdf_integrate_cell* q = nullptr;
    if (outCells && !S.cells.empty()) {
        q = (hpsdf_integrate_cell*)std::malloc(S.cells.size() * sizeof(IntegrateCell));
        if (!q) return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_clearance: host allocation failed");
        std::memcpy(q, S.cells.data(), S.cells.size() * sizeof(IntegrateCell));
    }
    *out = S.r;
    if (outCells) *outCells = q, *outCount = S.cells.size();
    return HPSDF_OK;
}

// what hpsdf_clearance_* reject before anything runs (0: fine)
int clearanceArgumentError(const double* pose, double isoA, uint32_t depth, double tol, uint32_t maxCells, uint32_t maxLeaves, const void* out,
                           const void* outCells, const void* outCount);

// what hpsdf_clearance_batch_* reject before anything runs (0: fine): clearanceArgumentError for every pose, decide, max_total_cells, n
int clearanceBatchArgumentError(const double* poses, size_t n, double isoA, uint32_t depth, double tol, double decide, uint32_t maxCells,
                                uint32_t maxLeaves, uint32_t maxTotalCells, const void* out);

// Clearance on the calling thread over the host arrays of tA and tB (clearance_host.cpp)
int hostClearance(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const PairArgs& p, const ClearanceArgs& a, hpsdf_clearance* out,
                  hpsdf_integrate_cell** outCells, uint64_t* outCount);

// the batch on the calling thread: hostClearance for every pose with a.decide; out is written only when every pose succeeded
int hostClearanceBatch(const ClsTree& tA, size_t nNodesA, const ClsTree& tB, const double* poses, size_t n, double isoA, uint32_t maxLeaves,
                       const ClearanceArgs& a, hpsdf_clearance* out);

}  // namespace hpsdf
