// The lattice arguments (lo, hi, n) of the calls that work on a lattice -- hpsdf_extract_surface, hpsdf_extract_surface_sparse (through
// surface_common.hpp) and hpsdf_query_bounds_grid_* (tree_bound.hpp) -- checked against a tree's root map in one place, so that every
// call derives the same spacing and refuses the same boxes.  Host only, header only, no HIP: the device-free entry points include it too.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "runtime.hpp"
#include "hpsdf.h"

namespace hpsdf {

namespace {

struct LatticeLimits {
    int axisLog2;    // n[a] <= 2^axisLog2 (32: no limit of its own)
    int pointsLog2;  // lattice points <= 2^pointsLog2
};
constexpr LatticeLimits kDenseLimits = {32, 30}, kSparseLimits = {20, 40};
constexpr LatticeLimits kBoundsLimits = {32, 40};  // (hpsdf_query_bounds_grid_*: the caller also holds the number of cubes to 2^32)

struct CheckedLattice {
    double lo[3], h[3];
    uint32_t n[3];
    uint64_t nPts, nCubes;
};

inline bool inRoot(const double* rc, const double* ris, int a, double x) {  // Query's f32 containment test (leaf_eval.hpp) on one coordinate
    const float f = (float)((x - rc[a]) * ris[a]);
    return f >= -0.5f && f <= 0.5f;
}

// The lattice arguments of an entry point named `what`, against a tree's root map (rootCentre, rootInvSizes).  Order of the checks:
// iso; per axis finite, lo < hi, n; the number of points; per axis the containment test.
inline int checkLattice(const char* what, const LatticeLimits& lim, const double* rc, const double* ris, const double* lo, const double* hi,
                        const uint32_t* n, double iso, CheckedLattice* out) {
    static const char* kAxis[3] = {"x", "y", "z"};
    const auto bad = [what](const std::string& msg) { return fail(HPSDF_ERR_INVALID_ARGUMENT, std::string(what) + ": " + msg); };
    const auto badAxis = [&](int a, const std::string& msg) { return bad(std::string("axis ") + kAxis[a] + ": " + msg); };
    if (!std::isfinite(iso)) return bad("iso must be finite");
    CheckedLattice g{};
    g.nPts = 1, g.nCubes = 1;
    bool tooMany = false;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) return badAxis(a, "lo and hi must be finite");
        if (!(lo[a] < hi[a])) return badAxis(a, "lo must be below hi");
        if (n[a] < 1) return badAxis(a, "n must be at least 1");
        if (n[a] > (1ull << lim.axisLog2)) return badAxis(a, "n must be at most 2^" + std::to_string(lim.axisLog2));
        if (!tooMany) {  // (a product within the limit times a factor below 2^33 stays below 2^64)
            g.nPts *= (uint64_t)n[a] + 1u;
            g.nCubes *= n[a];
            tooMany = g.nPts > (1ull << lim.pointsLog2);
        }
        g.lo[a] = lo[a];
        g.h[a] = (hi[a] - lo[a]) / (double)n[a];
        g.n[a] = n[a];
    }
    if (tooMany) return bad("more than 2^" + std::to_string(lim.pointsLog2) + " lattice points");
    for (int a = 0; a < 3; ++a) {
        // the containment test is monotone along an axis: the two extreme lattice points decide for all of them
        const double last = g.lo[a] + (double)n[a] * g.h[a];
        if (!inRoot(rc, ris, a, g.lo[a]) || !inRoot(rc, ris, a, last))
            return badAxis(a, "the box leaves the tree's root (Query would return DBL_MAX there)");
    }
    *out = g;
    return HPSDF_OK;
}

}  // namespace

}  // namespace hpsdf
