// Integrate (include/hpsdf.h, "Integrate"): the plain C++ part -- a cell's arithmetic, its classification, its contribution, the
// reduction rule, the level loop and the world transform.  Shared by integrate.hip (the kernels call cellClass and cellRow, the driver
// runs integrateLevels over device lists) and by host_query.cpp (the same loop over host lists): one set of statements with a fixed
// association, built with -ffp-contract=off, so host and device give the same bits.  No HIP compiler is needed for this file (the
// device-free entry and the sanitizer build compile it with g++).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tree_bound.hpp"

namespace hpsdf {

// a cell as every list and the optional output hold it: i, j, k at the absolute depth `depth` (hpsdf_integrate_cell, include/hpsdf.h)
struct IntegrateCell {
    uint32_t node;
    uint8_t depth;
    uint8_t cls;
    uint16_t i, j, k;
};
static_assert(sizeof(IntegrateCell) == 12 && sizeof(hpsdf_integrate_cell) == 12, "a cell is 12 bytes");

struct IntegrateArgs {
    double iso;
    uint32_t depth, samples, maxCells;
};

// A row of sums.  0: unit_volume_lo; 1: the undecided volume; 2: M0; 3-5: M1; 6-11: M2 (xx yy zz xy xz yz); 12-14: inside, outside and
// undecided final cells (counts below 2^53 are exact in a double and go through the same reduction).
constexpr int kIntRow = 15;
enum { kIntLo = 0, kIntUnd = 1, kIntM0 = 2, kIntCellsIn = 12, kIntCellsOut = 13, kIntCellsUnd = 14 };
constexpr int kIntBlock = 256;  // rows of a block of the reduction

// what hpsdf_integrate_* reject before anything runs (0: fine)
int integrateArgumentError(double iso, uint32_t depth, uint32_t samples, uint32_t maxCells, const void* out, const void* outCells, const void* outCount);

// List 0: the leaves a walk from the root reaches, in increasing node index, each with its depth and its integer coordinates there
// (child c of a node at (i, j, k) is at (2 i + (c & 1), 2 j + ((c >> 1) & 1), 2 k + (c >> 2))).  Integers only.
inline void integrateLeafCells(const NodeRec* recs, size_t nNodes, std::vector<IntegrateCell>& out) {
    std::vector<IntegrateCell> all(nNodes, IntegrateCell{0, 0xFF, 0, 0, 0, 0});
    std::vector<uint32_t> stack{0u};
    all[0] = IntegrateCell{0, 0, 0, 0, 0, 0};
    while (!stack.empty()) {
        const uint32_t n = stack.back();
        stack.pop_back();
        const NodeRec rec = recs[n];
        const IntegrateCell p = all[n];
        if (rec.b != kInteriorTag || p.depth >= HPSDF_TREE_MAX_DEPTH || rec.a >= nNodes || nNodes - rec.a < 8u) continue;
        for (uint32_t c = 0; c < 8u; ++c) {
            const uint32_t ch = rec.a + c;
            if (all[ch].depth != 0xFF) continue;  // (no validated tree reaches a node twice)
            all[ch] = IntegrateCell{ch, (uint8_t)(p.depth + 1), 0, (uint16_t)(2u * p.i + (c & 1u)), (uint16_t)(2u * p.j + ((c >> 1) & 1u)),
                                    (uint16_t)(2u * p.k + (c >> 2))};
            stack.push_back(ch);
        }
    }
    out.clear();
    for (size_t n = 0; n < nNodes; ++n)
        if (all[n].depth != 0xFF && recs[n].b <= 12u) out.push_back(all[n]);
}

// the cell's box in its leaf's unit coordinates at relative level `level`: lo_k = -1 + i_k 2^(1-l) (i_k: the low l bits of the absolute
// coordinate), hi_k = lo_k + 2^(1-l); all exact
__host__ __device__ inline void integrateCellLo(const IntegrateCell& c, int level, double (&lo)[3], double& w) {
    const uint32_t mask = (1u << level) - 1u;
    w = 2.0 / (double)(1u << level);
    lo[0] = -1.0 + (double)(c.i & mask) * w;
    lo[1] = -1.0 + (double)(c.j & mask) * w;
    lo[2] = -1.0 + (double)(c.k & mask) * w;
}

// Class of a cell (include/hpsdf.h, "Classifying a cell"): 1 outside, 2 inside, 0 undecided.  *finite: f_c and e are both finite.
template <class Eval>
__host__ __device__ inline uint32_t integrateCellClass(const ClsTree& t, const IntegrateCell& c, int level, double iso, const Eval& eval, bool* finite) {
    double lo[3], w;
    integrateCellLo(c, level, lo, w);
    double uc[3];
    for (int k = 0; k < 3; ++k) uc[k] = 0.5 * (lo[k] + (lo[k] + w));
    const double rho = 1.0 / (double)(1u << level);
    const NodeRec rec = t.nodes[c.node];
    const double fc = eval(t.coeffs + rec.a, (int)rec.b, uc[0], uc[1], uc[2], (int)c.depth - level);
    const double* K = t.consts + 4 * (size_t)c.node;
    const double e = HPSDF_SURFACE_SLACK * ((rho * K[0] + rho * K[1]) + rho * K[2]) + HPSDF_SURFACE_ETA * K[3];
    *finite = boundsFinite(fc) && boundsFinite(e);
    if (fc - iso > e) return 1u;
    if (iso - fc > e) return 2u;
    return 0u;
}

// the moments of a box of edge s and volume v centred at c: M0, M1[3], M2[6]
__host__ __device__ inline void integrateBoxMoments(double v, const double (&c)[3], double s, double (&m)[10]) {
    const double t = (s * s) / 12.0;
    m[0] = v;
    for (int k = 0; k < 3; ++k) m[1 + k] = v * c[k];
    for (int k = 0; k < 3; ++k) m[4 + k] = v * (c[k] * c[k] + t);
    m[7] = v * (c[0] * c[1]);
    m[8] = v * (c[0] * c[2]);
    m[9] = v * (c[1] * c[2]);
}

// The row of a FINAL cell (include/hpsdf.h, "A final cell"); c.cls holds its class.  eval is called from one place.
template <class Eval>
__host__ __device__ inline void integrateCellRow(const ClsTree& t, const IntegrateCell& c, int level, double iso, uint32_t q, const Eval& eval,
                                                 double (&row)[kIntRow]) {
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
    const NodeRec rec = t.nodes[c.node];
    const uint32_t count = 1u << (3u * shift);
    for (uint32_t n = 0; n < count; ++n) {  // x fastest, then y, then z
        const uint32_t idx[3] = {n & (q - 1u), (n >> shift) & (q - 1u), n >> (2u * shift)};
        double u[3], p[3];
        for (int k = 0; k < 3; ++k) {
            const double odd = (double)(2u * idx[k] + 1u);
            u[k] = lo[k] + odd * hu;
            p[k] = plo[k] + odd * hs;
        }
        const double f = eval(t.coeffs + rec.a, (int)rec.b, u[0], u[1], u[2], (int)c.depth - level);
        if (f < iso) {
            integrateBoxMoments(vs, p, ss, m);
            for (int k = 0; k < 10; ++k) row[kIntM0 + k] = row[kIntM0 + k] + m[k];
        }
    }
}

// child ch of a cell (x fastest)
__host__ __device__ inline IntegrateCell integrateChild(const IntegrateCell& c, uint32_t ch) {
    return IntegrateCell{c.node, (uint8_t)(c.depth + 1u), 0, (uint16_t)(2u * c.i + (ch & 1u)), (uint16_t)(2u * c.j + ((ch >> 1) & 1u)),
                         (uint16_t)(2u * c.k + (ch >> 2))};
}

// The reduction rule on the host: x holds kIntBlock rows (zero-padded by the caller); the block's sum ends in x[0].
inline void integrateBlockTree(double (*x)[kIntRow]) {
    for (int stride = kIntBlock / 2; stride >= 1; stride >>= 1)
        for (int t = 0; t < stride; ++t)
            for (int k = 0; k < kIntRow; ++k) x[t][k] = x[t][k] + x[t + stride][k];
}

// n rows (n * kIntRow doubles) -> one, by blocks of kIntBlock, pass after pass
inline void integrateReduceRows(std::vector<double>& rows, double (&out)[kIntRow]) {
    size_t n = rows.size() / kIntRow;
    std::vector<double> next;
    double x[kIntBlock][kIntRow];
    if (n == 0) {
        for (int k = 0; k < kIntRow; ++k) out[k] = 0.0;
        return;
    }
    do {
        next.clear();
        for (size_t b = 0; b < n; b += kIntBlock) {
            const size_t m = n - b < (size_t)kIntBlock ? n - b : (size_t)kIntBlock;
            std::memset(x, 0, sizeof x);
            std::memcpy(x, rows.data() + b * kIntRow, m * kIntRow * sizeof(double));
            integrateBlockTree(x);
            next.insert(next.end(), x[0], x[0] + kIntRow);
        }
        rows.swap(next);
        n = rows.size() / kIntRow;
    } while (n > 1);
    for (int k = 0; k < kIntRow; ++k) out[k] = rows[k];
}

// What the level loop leaves: the normalised sums and, when asked for, the final cells
struct IntegrateSums {
    double total[kIntRow];
    uint64_t listCells = 0;  // cells of all lists: one classification each
    uint32_t status = HPSDF_INTEGRATE_OK, levels = 0;
    std::vector<IntegrateCell> cells;
};

// The level loop (include/hpsdf.h, "Building the lists").  Lists: classify(level, n, &nSplit, &finite) classifies the n cells of the
// current list and counts those to split; contribute(level, n, nSplit, cells, T) makes the next list (nSplit == 0: none), appends the
// final cells to *cells when it is not null and returns the level's total row T; the next list then becomes the current one.
template <class Lists>
int integrateLevels(Lists& L, const IntegrateArgs& a, uint32_t n0, bool wantCells, IntegrateSums& S) {
    for (int k = 0; k < kIntRow; ++k) S.total[k] = 0.0;
    uint32_t n = n0;
    for (int level = 0;; ++level) {
        uint32_t nSplit = 0;
        bool finite = true;
        if (const int rc = L.classify(level, n, &nSplit, &finite)) return rc;
        S.listCells += n;
        S.levels = (uint32_t)level;
        if (!finite) {
            S.status = HPSDF_INTEGRATE_NOT_FINITE;
            S.cells.clear();
            return HPSDF_OK;
        }
        if (8ull * nSplit > a.maxCells) {  // the next list would not fit: this level is final
            S.status = HPSDF_INTEGRATE_CELL_LIMIT;
            nSplit = 0;
        }
        double T[kIntRow];
        if (const int rc = L.contribute(level, n, nSplit, wantCells ? &S.cells : nullptr, T)) return rc;
        for (int k = 0; k < kIntRow; ++k) S.total[k] = level == 0 ? T[k] : S.total[k] + T[k];
        if (nSplit == 0) return HPSDF_OK;
        n = 8u * nSplit;
    }
}

// The struct from the sums: the world frame by x_k = rootCentre_k + p_k size_k (include/hpsdf.h, "The world-frame results")
inline void integrateResult(const IntegrateSums& S, const double* rootCentre, const double* rootInvSizes, uint32_t q, hpsdf_integral* o) {
    std::memset(o, 0, sizeof *o);
    o->status = S.status, o->levels = S.levels;
    const double size[3] = {1.0 / rootInvSizes[0], 1.0 / rootInvSizes[1], 1.0 / rootInvSizes[2]};
    const double J = (size[0] * size[1]) * size[2];
    if (S.status == HPSDF_INTEGRATE_NOT_FINITE) {
        const double nan = boundsQuietNaN();
        o->unit_volume_lo = 0.0, o->unit_volume_hi = 1.0, o->unit_volume = nan;
        o->volume_lo = 0.0, o->volume_hi = J, o->volume = nan;
        for (int k = 0; k < 3; ++k) o->m1[k] = o->unit_m1[k] = nan;
        for (int k = 0; k < 6; ++k) o->m2[k] = o->unit_m2[k] = nan;
        return;
    }
    const double* T = S.total;
    const double M0 = T[kIntM0];
    const double* M1 = T + kIntM0 + 1;
    const double* M2 = T + kIntM0 + 4;
    o->unit_volume_lo = T[kIntLo];
    o->unit_volume_hi = T[kIntLo] + T[kIntUnd];
    o->unit_volume = M0;
    o->volume_lo = J * o->unit_volume_lo, o->volume_hi = J * o->unit_volume_hi, o->volume = J * M0;
    for (int k = 0; k < 3; ++k) {
        o->unit_m1[k] = M1[k];
        o->m1[k] = J * (rootCentre[k] * M0 + size[k] * M1[k]);
    }
    const int ja[6] = {0, 1, 2, 0, 0, 1}, ka[6] = {0, 1, 2, 1, 2, 2};
    for (int n = 0; n < 6; ++n) {
        const int j = ja[n], k = ka[n];
        o->unit_m2[n] = M2[n];
        o->m2[n] = J * (((rootCentre[j] * rootCentre[k]) * M0 + (rootCentre[j] * size[k]) * M1[k]) +
                        ((rootCentre[k] * size[j]) * M1[j] + (size[j] * size[k]) * M2[n]));
    }
    o->cells_inside = (uint64_t)T[kIntCellsIn], o->cells_outside = (uint64_t)T[kIntCellsOut], o->cells_undecided = (uint64_t)T[kIntCellsUnd];
    o->evaluations = S.listCells + o->cells_undecided * (uint64_t)(q * q * q);
}

// the struct and the optional malloc'd cell array into the caller's outputs (hpsdf_extract_surface's convention: an empty result is NULL, 0)
inline int integrateHandOver(const IntegrateSums& S, const hpsdf_integral& r, hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
    hpsdf_integrate_cell* p = nullptr;
    if (outCells && !S.cells.empty()) {
        p = (hpsdf_integrate_cell*)std::malloc(S.cells.size() * sizeof(IntegrateCell));
        if (!p) return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_integrate: host allocation failed");
        std::memcpy(p, S.cells.data(), S.cells.size() * sizeof(IntegrateCell));
    }
    *out = r;
    if (outCells) *outCells = p, *outCount = S.cells.size();
    return HPSDF_OK;
}

// integrateLevels' lists on the calling thread.  Cells gives a cell's class and a final cell's row: cls(c, level, &finite), row(c, level, row)
// (Integrate's: host_query.cpp; IntegratePair's: integrate_pair_host.cpp).
template <class Cells>
struct HostIntegrateLists {
    Cells& cells;
    uint32_t maxDepth;
    std::vector<IntegrateCell> cur, next;
    std::vector<uint8_t> split;
    std::vector<double> rows;

    int classify(int level, uint32_t n, uint32_t* nSplit, bool* finite) {
        split.assign(n, 0);
        uint32_t count = 0;
        for (uint32_t i = 0; i < n; ++i) {
            bool ok = true;
            IntegrateCell& c = cur[i];
            c.cls = (uint8_t)cells.cls(c, level, &ok);
            if (!ok) *finite = false;
            split[i] = c.cls == 0u && c.depth < maxDepth;
            count += split[i];
        }
        *nSplit = count;
        return HPSDF_OK;
    }

    int contribute(int level, uint32_t n, uint32_t nSplit, std::vector<IntegrateCell>* finals, double (&T)[kIntRow]) {
        next.clear();
        next.reserve(8 * (size_t)nSplit);
        rows.clear();
        double x[kIntBlock][kIntRow];
        for (uint32_t b = 0; b < n; b += kIntBlock) {
            std::memset(x, 0, sizeof x);
            for (uint32_t i = b; i < n && i < b + kIntBlock; ++i) {
                const IntegrateCell& c = cur[i];
                if (nSplit != 0 && split[i]) {
                    for (uint32_t ch = 0; ch < 8u; ++ch) next.push_back(integrateChild(c, ch));
                    continue;
                }
                cells.row(c, level, x[i - b]);
                if (finals) finals->push_back(c);
            }
            integrateBlockTree(x);
            rows.insert(rows.end(), x[0], x[0] + kIntRow);
        }
        integrateReduceRows(rows, T);
        cur.swap(next);
        return HPSDF_OK;
    }
};

// The call on the calling thread: list 0 of t, the level loop, the struct and the cells
template <class Cells>
int hostIntegrateLists(Cells& cells, const ClsTree& t, size_t nNodes, const IntegrateArgs& a, hpsdf_integral* out, hpsdf_integrate_cell** outCells,
                       uint64_t* outCount) {
    HostIntegrateLists<Cells> L{cells, a.depth, {}, {}, {}, {}};
    integrateLeafCells(t.nodes, nNodes, L.cur);
    IntegrateSums S;
    if (const int rc = integrateLevels(L, a, (uint32_t)L.cur.size(), outCells != nullptr, S)) return rc;
    hpsdf_integral r;
    integrateResult(S, t.rootCentre, t.rootInvSizes, a.samples, &r);
    return integrateHandOver(S, r, out, outCells, outCount);
}

// Integrate on the calling thread over the host arrays of t (host_query.cpp)
int hostIntegrate(const ClsTree& t, size_t nNodes, const IntegrateArgs& a, hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount);

}  // namespace hpsdf
