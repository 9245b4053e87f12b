// Evaluation of trees at points: the gfx950 Query kernels (Octree::Query + FApprox, Octree.cpp:662-702, 859-901) -- the headline
// query_kernel, the general / LDS / deferred / few-point kernels, their gradient versions, rays, slices, the surface lattice -- and
// their launchers; the leaf evaluation and the descent they share with the fit's CSG wrapper are leaf_eval.hpp.
// fit_weight_kernel (mean FApprox of freshly fitted leaves) is here too: it calls evalLeafGeneric, which is not inlined, and in a
// unit where it is the only caller the compiler specialises that function for it and both come out as different code.
// The name kernels.hip stays although the fits and the mesh kernels live in fit*.hip and mesh_field.hip: bench.py and
// tools/check_evidence_stamps.py hash the text from queryTopBody to query_grad_kernel below, in csrc/kernels.hip, to tell whether
// profiles/query_pmc.json still describes the headline kernel.
//
// Built with -ffp-contract=off: the reference CPU path runs on baseline x86-64
// (no FMA), so every multiply-add below is a separate v_mul_f64 / v_add_f64 and
// every sum runs in the reference's order.  That makes the GPU results
// bit-identical to the CPU restatement (oracle/), which is what keeps the
// octree topology identical (near-ties in the refinement decisions and in the
// heap order would otherwise flip on 1-ulp differences).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>

#include "device_types.hpp"
#include "field_eval.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"

namespace hpsdf {

// Batched Query, trees whose leaves ALL sit in the top table with degree <= 2 (what the BASELINE thresholds
// produce: 4096 depth-4 leaves of degree 2).  Random points share nothing, so per point the tree costs one
// 128-byte top-table line out of L2; fetched lane-by-lane that is 6 divergent 16-byte requests per point and the
// texture addresser becomes the limit.  Here the wave fetches cooperatively: in step k the 8 lanes of every
// group read the 8 consecutive 16-byte chunks of the line of the group's k-th point, straight into LDS
// (global_load_lds_dwordx4: lane-linear destination, per-lane source), i.e. 8 whole lines per
// wave-instruction instead of 64 fragments; afterwards every lane reads back its own point's row.
// Every other tree goes through query_general_kernel below.
// GRAD: QueryWithGradient (Octree.cpp:749-789, 904-985) on the same trees -- the same fetch, value and "gradient" from the row
// (evalLeafGradVals); rows of grad for points outside the root are left untouched, as the reference leaves its output argument.
template <int TOPD, bool DEDUPE, bool GRAD>
__device__ __forceinline__ void queryTopBody(const TreeDev& t, const double* __restrict__ xyz, size_t n, double* __restrict__ out,
                                             double* __restrict__ grad, const double* sNl, const double* sRec) {
    // per wave: 4 steps x 64 lanes x 16 B (two passes; less LDS = more waves).  Each step's kilobyte is followed by
    // 32 bytes of padding: a lane reads row (sub & 3), so without it the four lanes of a group hit the same banks
    // one kilobyte apart (measured: 70 % of the LDS cycles were bank conflicts).
    __shared__ double2 sRows[4][4][66];
    __shared__ uint32_t sRunCell[4][64];  // ordered input: the cell of every run of equal cells in the wave (below)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane & ~7, sub = lane & 7;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        const size_t i = base + threadIdx.x;
        const bool valid = i < n;
        const size_t il = valid ? i : n - 1;
        // (plain loads: non-temporal ones, 3 x 8 bytes or 16 + 8, cost the kernel 30 us -- neighbouring lanes share the points' lines, and
        // without the caches every lane fetches them for itself; the RESULTS leave non-temporally: below)
        const double x = xyz[3 * il], y = xyz[3 * il + 1], z = xyz[3 * il + 2];
        // Octree.cpp:665
        const double p3[3] = {(x - t.rootCentre[0]) * t.rootInvSizes[0], (y - t.rootCentre[1]) * t.rootInvSizes[1],
                              (z - t.rootCentre[2]) * t.rootInvSizes[2]};
        // :668 containment on the f32 cast, both ends inclusive; NaN fails
        const float fx = (float)p3[0], fy = (float)p3[1], fz = (float)p3[2];
        const bool inside = fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f;
        const int topDepth = TOPD > 0 ? TOPD : t.topDepth;
        int k3[3];
        double c3[3];
        topCell(p3, topDepth, k3, c3);
        uint32_t code = (uint32_t)(k3[0] + ((k3[1] + (k3[2] << topDepth)) << topDepth));
        if (!inside) code = 0;  // any valid line; the result is DBL_MAX
        // lane (group g, sub k) owns the row that step k writes at lanes 8g..8g+7: [record][c0 c1]..[c8 c9].
        // Two passes of four steps through a 4 KB per-wave window (measured: 110 vs 121 us for one 8 KB pass).
        // Points of a group that fall into the same cell share one fetch: step k runs for a group only if its k-th
        // point is the first of the group in its cell, and every lane reads the row of the first point of its own cell
        // (coherent point sets -- grids, slices, rays -- move a fraction of the lines; random points lose nothing but a
        // few compares: the kernel is bound by the L2 -> CU line traffic).
        uint2 hdr = make_uint2(0u, 0u);
        double cv[10];
        // ORDERED INPUT (round 6).  Grids, slices, rays and cell-sorted point sets arrive as RUNS of consecutive points in one cell: a
        // lane opens a run if its cell differs from the lane's before it.  With at most 32 runs in the wave -- random points have 64 --
        // the wave needs one row per RUN, not one per point or per group of eight: the lanes that open a run publish its cell, step s
        // fetches the rows of runs 8s .. 8s + 7 (eight lanes a row, as ever), and every lane reads back the row of its own run; four steps at
        // most, one for a wave that crosses a handful of cells, and no second pass.  A wave that lies in ONE cell altogether -- the rule in
        // cell-sorted sets, 2 441 points a cell at 10 M points -- asks for its row through the scalar cache and evaluates from SGPRs: no
        // LDS, no vector memory at all.  The rows are the same bytes whichever way they come, so the values are too
        // (test_query_ordered_point_sets_bitwise).  What the group-wise dedupe of rounds 1-5 cost such sets was its bookkeeping: eight
        // shuffles and ~60 compares a tile on a kernel whose arithmetic is 228 vector instructions a tile and which, on ordered input, is
        // bound by exactly that.
        bool viaRuns = false;
        if (DEDUPE) {
            const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp((int)code, (int)code, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            const bool opens = lane == 0 || before != code;
            const unsigned long long heads = __ballot(opens);
            const int nRuns = __popcll(heads);  // wave-uniform
            if (nRuns == 1) {
                const uint32_t cell = (uint32_t)__builtin_amdgcn_readfirstlane((int)code);
                typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
                const ConstWords w = (ConstWords)(uintptr_t)(t.top + cell);
                hdr = make_uint2(w[0], w[1]);
#pragma unroll
                for (int c = 0; c < 10; ++c) cv[c] = __longlong_as_double((long long)(((unsigned long long)w[5 + 2 * c] << 32) | (unsigned long long)w[4 + 2 * c]));
                viaRuns = true;
            } else if (nRuns <= 32) {
                // (the wave's row of sRunCell from an index the compiler cannot see through: hoisted out of the tile loop, that address is
                // one register more than the kernel's seven waves a SIMD leave it, and it went to scratch)
                uint32_t waveV = (uint32_t)threadIdx.x >> 6;
                asm volatile("" : "+v"(waveV));
                uint32_t* runCell = sRunCell[waveV];
                const uint32_t myRun = __builtin_amdgcn_mbcnt_hi((uint32_t)(heads >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)heads, 0u)) + (opens ? 1u : 0u) - 1u;
                if (opens) runCell[myRun] = code;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                const int nSteps = (nRuns + 7) >> 3;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < nSteps) {
                        const int run = 8 * k + (lane >> 3);
                        if (run < nRuns && sub < 6) {  // bytes 96..127 of an entry are padding
                            const char* src = reinterpret_cast<const char*>(t.top + runCell[run]) + sub * 16;
                            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                             (__attribute__((address_space(3))) void*)&sRows[wave][k][0], 16, 0, 0);
                        }
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                {
                    const double2* row = &sRows[wave][myRun >> 3][(myRun & 7u) * 8u];
                    hdr = *reinterpret_cast<const uint2*>(row);
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        const double2 v = row[1 + c];
                        cv[2 * c] = v.x;
                        cv[2 * c + 1] = v.y;
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();  // the window is rewritten by the next tile
                viaRuns = true;
            }
        }
        if (!viaRuns) {
        uint32_t ck[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) ck[k] = __shfl(code, grp | k, 64);
        int firstOfMine = sub;  // first point of the group in this lane's cell
        uint32_t needMask = 0xFFu;  // bit k: point k is the first of its cell in the group
        // wave-uniform gate: on random points (almost) no wave has two neighbouring lanes in one cell and the
        // bookkeeping below is skipped; on point sets with SOME order (more than 32 runs, yet neighbours that share cells) it pays
        if (DEDUPE && __any(__shfl_xor(code, 1, 64) == code)) {
#pragma unroll
            for (int k = 7; k >= 0; --k) firstOfMine = ck[k] == code ? k : firstOfMine;
            needMask = 1u;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                bool seen = false;
#pragma unroll
                for (int j = 0; j < k; ++j) seen = seen || (ck[j] == ck[k]);
                needMask |= seen ? 0u : (1u << k);
            }
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const char* src = reinterpret_cast<const char*>(t.top + ck[pass * 4 + k]) + sub * 16;
                if (sub < 6 && ((needMask >> (pass * 4 + k)) & 1u))  // bytes 96..127 of an entry are padding
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)&sRows[wave][k][0], 16, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if ((firstOfMine >> 2) == pass) {
                const double2* row = &sRows[wave][firstOfMine & 3][grp];
                hdr = *reinterpret_cast<const uint2*>(row);
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const double2 v = row[1 + c];
                    cv[2 * c] = v.x;
                    cv[2 * c + 1] = v.y;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();  // the window is rewritten by the next pass / tile
        }
        }
        double r = DBL_MAX;  // :668-671 outside the root
        if constexpr (GRAD) {
            double g[3] = {0.0, 0.0, 0.0};
            if (inside) {
                const double s = (double)(2 << topDepth);  // :862
                const double u[3] = {(p3[0] - c3[0]) * s, (p3[1] - c3[1]) * s, (p3[2] - c3[2]) * s};
                if (hdr.y == 2u)
                    r = evalLeafGradVals<2>(cv, u, topDepth, sNl, sRec, g, t.leftAssoc);
                else if (hdr.y == 1u)
                    r = evalLeafGradVals<1>(cv, u, topDepth, sNl, sRec, g, t.leftAssoc);
                else
                    r = evalLeafGradVals<0>(cv, u, topDepth, sNl, sRec, g, t.leftAssoc);
            }
            if (valid) {
                __builtin_nontemporal_store(r, &out[i]);
                if (inside) {
                    __builtin_nontemporal_store(g[0], &grad[3 * i]);
                    __builtin_nontemporal_store(g[1], &grad[3 * i + 1]);
                    __builtin_nontemporal_store(g[2], &grad[3 * i + 2]);
                }
            }
        } else {
            if (inside) {
                // :862  unitPt = (pt - centre) * (2 << depth)
                const double s = (double)(2 << topDepth);
                const double ux = (p3[0] - c3[0]) * s, uy = (p3[1] - c3[1]) * s, uz = (p3[2] - c3[2]) * s;
                // (the normalisation factors through a barrier the optimiser cannot see through: it hoists nl[0]^2 and nl[0]^3 out of the
                // tile loop otherwise, into registers that the kernel's seven waves a SIMD do not have -- they went to scratch and came
                // back once a tile; one multiply a tile is cheaper than one memory operation)
                double nlT[3] = {t.nlTop[0], t.nlTop[1], t.nlTop[2]};
                asm volatile("" : "+s"(nlT[0]));
                if (hdr.y == 2u)
                    r = evalLeafTop<2>(cv, ux, uy, uz, nlT);
                else if (hdr.y == 1u)
                    r = evalLeafTop<1>(cv, ux, uy, uz, nlT);
                else
                    r = evalLeafTop<0>(cv, ux, uy, uz, nlT);
            }
            if (valid) __builtin_nontemporal_store(r, &out[i]);
        }
    }
}

template <int TOPD, bool DEDUPE>
__global__ __launch_bounds__(256, 7) void query_kernel(TreeDev t, const double* __restrict__ xyz, size_t n,
                                                    double* __restrict__ out) {
    queryTopBody<TOPD, DEDUPE, false>(t, xyz, n, out, nullptr, nullptr, nullptr);
}

// QueryWithGradient on the trees query_kernel serves (every leaf in the top table, degree <= 2): one line a point like Query, where
// the any-tree kernel (query_general_grad_kernel) pays a record lookup, a walk and a second round trip.
template <int TOPD>
__global__ __launch_bounds__(256, 4) void query_grad_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                            size_t n, double* __restrict__ out, double* __restrict__ grad) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    queryTopBody<TOPD, true, true>(t, xyz, n, out, grad, sNl, sRec);
}

// 16-byte chunks a leaf of degree d occupies in the device mirror (blocks are 128-byte aligned there)
__device__ __forceinline__ uint32_t leafChunks(uint32_t degree) { return ((uint32_t)coeffCount((int)degree) + 1u) >> 1; }

// Batched Query, any tree.  Per lane: the top cell by arithmetic, its 8-byte record from the thin top table
// (32 KB at depth 4: L1/L2 traffic only), then the walk down to the leaf (Octree.cpp:674-701).  The leaves'
// coefficients are then fetched by the wave as a whole, as in query_kernel, straight from the coefficient mirror
// (every leaf block starts on a 128-byte line there): in step k the 8 lanes of a group fetch chunks 0..7 of the
// leaf of the group's k-th point -- a whole degree-2 leaf, the first line of a degree-3 one -- and one extra step
// per pass brings chunks 8..9 of four degree-3 leaves at a time (two lanes each).  Two passes of 4 + 1 steps
// through a 5 KB per-wave window, i.e. two L2 round trips per tile whatever the mix of degrees <= 3 (one pass of
// 8 + 2 steps through a 10 KB window measured 3 % slower: fewer workgroups per CU).
// Leaves of degree > 3 are rare at the thresholds in use (a few dozen among thousands): DEFER appends their points to
// the workgroup's own run of deferIdx (an LDS counter, no global atomic -- one global atomic per wave serialised
// the first version of this at 2 ms per 10 M points) and query_deep_kernel finishes them lane by lane; keeping
// that code out of this kernel's loop keeps the loop at ~100 VGPRs (the 16-wave kernel has room up to 128, and finishes degrees 4-5
// itself behind its last tile: DEEP below).
// GRAD: QueryWithGradient (Octree.cpp:749-789) -- the same walk and fetch, value and "gradient" evaluated together;
// rows of grad for points outside the root are left untouched, as the reference leaves its output argument.
// WAVES: waves per workgroup (tile = 64 WAVES points).  LDSTOP (depth-4 top level only): the thin top table, 32 KB,
// sits in LDS -- the kernel runs at 4 waves per SIMD for its registers anyway, so one 16-wave workgroup per CU with
// ~120 KB of LDS costs no occupancy and takes the record lookup (an L2 round trip and 64 scattered 8-byte requests
// per wave) off the dependent chain.
constexpr size_t queryGeneralLdsBytes(int waves, bool ldsTop) {
    return (size_t)waves * 5 * 66 * sizeof(double2) + (size_t)waves * 64 * sizeof(uint32_t) + (ldsTop ? 4096 * sizeof(NodeRec) : 0);
}
// LAB (tools/query_general_floor.py, HPSDF_QUERY_LAB=n; results are NOT the tree's values): what the kernel's time is made of, by taking
// one link of its chain out at a time -- 1: no polynomial (the fetched rows are touched, not evaluated); 2: every lane fetches the leaf
// of its wave's first lane (the same instructions, but every line after the first is a hit: no gather traffic); 3: no second line for
// degree-3 leaves; 4: no walk below the top table (the top record is taken for the leaf)
// DEEP > 0 (values only, trees whose degrees stop at DEEP): the workgroup finishes its own deferred points behind its last tile, one lane
// each with queryPoint<DEEP> -- the lists are per workgroup, so nothing has to be scanned or waited for across workgroups, and the scan
// launch and the second pass (with the two kernel boundaries they bring: ~15 us behind a 176 us kernel for 10 M points on union3 @ 1e-7)
// are not launched at all.
template <int TOPD, bool DEFER, bool GRAD, int WAVES, bool LDSTOP, int LAB = 0, int DEEP = 0>
__device__ __forceinline__ void queryGeneralBody(const TreeDev& t, const DeviceTables* __restrict__ T,
                                                 const double* __restrict__ xyz, size_t n, double* __restrict__ out,
                                                 double* __restrict__ grad, uint32_t tilesPerWg,
                                                 uint32_t* __restrict__ deferCount, uint32_t* __restrict__ deferIdx) {
    static_assert(!LDSTOP || TOPD == 4, "the LDS copy of the thin table is sized for depth 4");
    constexpr int TILE = WAVES * 64;
    extern __shared__ double2 sDyn[];
    double2(*sRows)[5][66] = reinterpret_cast<double2(*)[5][66]>(sDyn);           // [WAVES][5][66]
    uint32_t(*sInfo)[64] = reinterpret_cast<uint32_t(*)[64]>(sDyn + WAVES * 5 * 66);  // [WAVES][64]
    NodeRec* sTop = reinterpret_cast<NodeRec*>(&sInfo[WAVES][0]);                  // [4096] when LDSTOP
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint32_t sDeferred;
    stageQueryTables(T, sNl, sRec);
    if constexpr (LDSTOP) {
        for (int q = threadIdx.x; q < 4096; q += TILE) sTop[q] = t.topRec[q];
    }
    if (threadIdx.x == 0) sDeferred = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane & ~7, sub = lane & 7;
    const size_t segStart = (size_t)blockIdx.x * tilesPerWg * TILE;  // this workgroup's run of deferIdx
    // The points of a tile are asked for while the previous tile still waits for its last coefficient fetch (below): a wave's tile is a
    // chain of dependent round trips -- points from HBM (~1.8 us under load), record, walk, two coefficient fetches from L2 (~0.8 us
    // each), ~0.5 us of arithmetic -- and with 16 waves on a CU the kernel runs at what that chain's length allows, not at a bandwidth
    // limit (profiles/r02w_query_general_counters.txt: the texture addresser is busy half of the time).  The first link now overlaps
    // the previous tile's last fetch and its evaluation.
    typedef double qg_double2 __attribute__((ext_vector_type(2)));
    qg_double2 nxy = {0.0, 0.0};
    double nz = 0.0;
    {
        const size_t i0 = (size_t)blockIdx.x * TILE + threadIdx.x;
        if ((size_t)blockIdx.x * TILE < n) {
            const size_t il0 = i0 < n ? i0 : n - 1;
            nxy.x = xyz[3 * il0], nxy.y = xyz[3 * il0 + 1], nz = xyz[3 * il0 + 2];
        }
    }
    for (size_t base = (size_t)blockIdx.x * TILE; base < n; base += (size_t)gridDim.x * TILE) {
        const size_t i = base + threadIdx.x;
        const bool valid = i < n;
        const double x = nxy.x, y = nxy.y, z = nz;
        const size_t nextBase = base + (size_t)gridDim.x * TILE;
        const bool more = nextBase < n;  // workgroup-uniform
        const double p3[3] = {(x - t.rootCentre[0]) * t.rootInvSizes[0], (y - t.rootCentre[1]) * t.rootInvSizes[1],
                              (z - t.rootCentre[2]) * t.rootInvSizes[2]};  // Octree.cpp:665
        const float fx = (float)p3[0], fy = (float)p3[1], fz = (float)p3[2];
        const bool inside = fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f;  // :668
        const int topDepth = TOPD > 0 ? TOPD : t.topDepth;
        int k3[3];
        double c3[3];
        topCell(p3, topDepth, k3, c3);
        uint32_t code = (uint32_t)(k3[0] + ((k3[1] + (k3[2] << topDepth)) << topDepth));
        if (!inside) code = 0;
        NodeRec rec = LDSTOP ? sTop[code] : t.topRec[code];
        int depth = topDepth;
        double q = 0.25 / (double)(1 << topDepth);  // a quarter of the cell size: from a centre to its children's
        if constexpr (LAB == 4) {
            if (rec.b == kInteriorTag) rec.a = 0, rec.b = 2;
        }
        while (rec.b == kInteriorTag) {              // :674-701 below the complete levels
            const bool ux = p3[0] >= c3[0], uy = p3[1] >= c3[1], uz = p3[2] >= c3[2];
            const uint32_t idx = rec.a + (ux ? 1u : 0u) + (uy ? 2u : 0u) + (uz ? 4u : 0u);
            c3[0] = ux ? c3[0] + q : c3[0] - q;
            c3[1] = uy ? c3[1] + q : c3[1] - q;
            c3[2] = uz ? c3[2] + q : c3[2] - q;
            q = q * 0.5;
            ++depth;
            rec = t.nodes[idx];
        }
        const uint32_t degree = rec.b;
        const bool coop = inside && degree <= 3u;
        // :862 / :907  unitPt = (pt - centre) * (2 << depth) -- formed now, so that the point and the centre need no
        // registers across the fetch
        const double sc = (double)(2 << depth);
        const double u[3] = {(p3[0] - c3[0]) * sc, (p3[1] - c3[1]) * sc, (p3[2] - c3[2]) * sc};
        // what the fetching lanes need to know about this lane's leaf: block offset (a multiple of 16 doubles, so its
        // low four bits are free) and chunk count (0 = nothing to fetch)
        const uint32_t infoMine = rec.a | (coop ? leafChunks(degree) : 0u);
        double cv[20];
        // ORDERED INPUT (round 6; as in queryTopBody).  Grids, slices, rays and sorted point sets reach this kernel as RUNS of consecutive
        // points in one leaf.  With at most 32 runs in the wave (random points: 64) the wave fetches one block per RUN in ONE pass -- step s
        // the first lines of runs 8s .. 8s + 7, one more step the second lines of up to 32 degree-3 leaves, two lanes each -- and every
        // lane reads back its run's block: one round trip to L2 instead of two on this kernel's chain of dependent round trips, and a
        // quarter of the window's traffic.  The same bytes whichever way they come (test_query_ordered_point_sets_bitwise).
        bool viaRuns = false;
        if constexpr (LAB == 0) {
            const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp((int)infoMine, (int)infoMine, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            const bool opens = lane == 0 || before != infoMine;
            const unsigned long long heads = __ballot(opens);
            const int nRuns = __popcll(heads);  // wave-uniform
            if (nRuns <= 32) {
                viaRuns = true;
                const uint32_t myRun = __builtin_amdgcn_mbcnt_hi((uint32_t)(heads >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)heads, 0u)) + (opens ? 1u : 0u) - 1u;
                if (opens) sInfo[wave][myRun] = infoMine;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                const int nSteps = (nRuns + 7) >> 3;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < nSteps) {
                        const int run = 8 * k + (lane >> 3);
                        const uint32_t inf = run < nRuns ? sInfo[wave][run] : 0u;
                        const char* src = reinterpret_cast<const char*>(t.coeffs) + (size_t)(inf & ~15u) * 8u + (uint32_t)sub * 16u;
                        if ((uint32_t)sub < (inf & 15u))
                            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                             (__attribute__((address_space(3))) void*)&sRows[wave][k][0], 16, 0, 0);
                    }
                }
                if (__any(coop && degree == 3u)) {  // chunks 8..9 of the runs' degree-3 leaves: two lanes a run
                    const int run = lane >> 1;
                    const uint32_t inf = run < nRuns ? sInfo[wave][run] : 0u;
                    const char* src = reinterpret_cast<const char*>(t.coeffs) + (size_t)(inf & ~15u) * 8u + (8u + (uint32_t)(lane & 1)) * 16u;
                    if ((inf & 15u) > 8u)
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                         (__attribute__((address_space(3))) void*)&sRows[wave][4][0], 16, 0, 0);
                }
                if (more) {  // the next tile's points behind the fetch, as below
                    const size_t in = nextBase + threadIdx.x;
                    const double* np = xyz + 3 * (in < n ? in : n - 1);
                    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx2 %1, %2, off offset:16\n\ts_waitcnt vmcnt(2)"
                                 : "=&v"(nxy), "=&v"(nz)
                                 : "v"(np)
                                 : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_wave_barrier();
                {
                    const double2* row = &sRows[wave][myRun >> 3][(myRun & 7u) * 8u];
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const double2 v = row[c];
                        cv[2 * c] = v.x;
                        cv[2 * c + 1] = v.y;
                    }
                    const double2* tail = &sRows[wave][4][2u * myRun];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const double2 v = tail[c];
                        cv[16 + 2 * c] = v.x;
                        cv[16 + 2 * c + 1] = v.y;
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();  // the window is rewritten by the next tile
            }
        }
        if (!viaRuns) {
        sInfo[wave][lane] = infoMine;
        __builtin_amdgcn_wave_barrier();
        if constexpr (LAB == 2) {
            const uint32_t first = sInfo[wave][0];
            __builtin_amdgcn_wave_barrier();
            sInfo[wave][lane] = first;
            __builtin_amdgcn_wave_barrier();
        }
        const bool second = LAB != 3 && __any(coop && degree == 3u);  // wave-uniform: somebody needs chunks 8..9
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // chunks 0..7 of the leaf of point (group, 4 pass + k)
                const uint32_t inf = sInfo[wave][grp + pass * 4 + k];
                const char* src = reinterpret_cast<const char*>(t.coeffs) + (size_t)(inf & ~15u) * 8u + (uint32_t)sub * 16u;
                if ((uint32_t)sub < (inf & 15u))
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)&sRows[wave][k][0], 16, 0, 0);
            }
            if (second) {  // chunks 8..9 of the leaves of points (group, 4 pass + 0..3): two lanes each
                const uint32_t inf = sInfo[wave][grp + 4 * pass + (sub >> 1)];
                const char* src = reinterpret_cast<const char*>(t.coeffs) + (size_t)(inf & ~15u) * 8u + (8u + (uint32_t)(sub & 1)) * 16u;
                if ((inf & 15u) > 8u)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)&sRows[wave][4][0], 16, 0, 0);
            }
            if (pass == 1 && more) {
                // the next tile's points, issued BEHIND this tile's last coefficient fetch: memory operations of a wave complete in
                // order, so "all but the two youngest" (vmcnt(2)) is exactly "the coefficients are in LDS", and the two point loads
                // stay in flight across the read-back and the evaluation (written out as instructions: the count in the wait must be
                // the number of loads, which the compiler is free to merge or split; the values are claimed further down, before the
                // stores, by a wait of their own).  Plain loads: until the end of round 5 these carried `nt`, which made every lane fetch the
                // lines its neighbours share for itself -- 193 -> 168 us on union3 @ 1e-7 without it.  The results do leave non-temporally.
                const size_t in = nextBase + threadIdx.x;
                const double* np = xyz + 3 * (in < n ? in : n - 1);
                asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx2 %1, %2, off offset:16\n\ts_waitcnt vmcnt(2)"
                             : "=&v"(nxy), "=&v"(nz)
                             : "v"(np)
                             : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_wave_barrier();
            if ((sub >> 2) == pass) {
                const double2* row = &sRows[wave][sub & 3][grp];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const double2 v = row[c];
                    cv[2 * c] = v.x;
                    cv[2 * c + 1] = v.y;
                }
                const double2* tail = &sRows[wave][4][grp + 2 * (sub & 3)];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double2 v = tail[c];
                    cv[16 + 2 * c] = v.x;
                    cv[16 + 2 * c + 1] = v.y;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();  // the window is rewritten by the next pass / tile
        }
        }
        double r = DBL_MAX;  // :668-671
        double g[3] = {0.0, 0.0, 0.0};
        bool defer = false;
        if (LAB == 1 && inside) {
            r = (cv[0] + cv[9]) + (cv[16] + cv[19]) + u[0] * u[1] + u[2] + (double)depth;
        } else if (inside) {
            if constexpr (GRAD) {
                if (degree > 3u)
                    defer = valid;
                else if constexpr (LAB == 5)  // (lab: the gradient kernel with the value's arithmetic only -- what the six one-sided sums, the divisions and the square root cost)
                    r = evalLeafValsMixed<3>(cv, u[0], u[1], u[2], depth, degree, sNl, sRec), g[0] = r, g[1] = u[1], g[2] = u[2];
                else
                    r = evalLeafGradValsMixed<3, 20, LAB == 6>(cv, u, depth, degree, sNl, sRec, g, t.leftAssoc);
            } else {
                // one pass for the wave's mix of degrees (evalLeafValsMixed)
                if (degree > 3u)
                    defer = valid;
                else
                    r = evalLeafValsMixed<3>(cv, u[0], u[1], u[2], depth, degree, sNl, sRec);
            }
        }
        // the next tile's points have had the evaluation's time to arrive: claim them before this tile's stores are issued (a wait
        // behind the stores would wait for those too)
        if (more) asm volatile("s_waitcnt vmcnt(0)" : "+v"(nxy), "+v"(nz)::"memory");
        if constexpr (DEFER) {
            const unsigned long long dmask = __ballot(defer);
            if (dmask) {  // one LDS atomic per wave reserves the slots
                uint32_t slot = 0;
                const int leader = __ffsll((long long)dmask) - 1;
                if (lane == leader) slot = atomicAdd(&sDeferred, (uint32_t)__popcll(dmask));
                slot = __shfl(slot, leader, 64);
                if (defer) deferIdx[segStart + slot + (uint32_t)__popcll(dmask & ((1ull << lane) - 1ull))] = (uint32_t)i;
            }
        }
        if (valid && !defer) {
            __builtin_nontemporal_store(r, &out[i]);
            if constexpr (GRAD) {
                if (inside) {
                    __builtin_nontemporal_store(g[0], &grad[3 * i]);
                    __builtin_nontemporal_store(g[1], &grad[3 * i + 1]);
                    __builtin_nontemporal_store(g[2], &grad[3 * i + 2]);
                }
            }
        }
    }
    if constexpr (DEFER && DEEP > 0) {
        static_assert(!GRAD, "the fused second pass writes values only");
        __syncthreads();  // every wave's indices are written (and visible inside the workgroup), the count is final
        const uint32_t nd = sDeferred;
        for (uint32_t j = threadIdx.x; j < nd; j += TILE) {
            const size_t i = deferIdx[segStart + j];
            __builtin_nontemporal_store(queryPoint<DEEP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], sNl, sRec), &out[i]);
        }
    } else if constexpr (DEFER) {
        __syncthreads();
        if (threadIdx.x == 0) deferCount[blockIdx.x] = sDeferred;
    }
}

// Values only: ~104 VGPRs, 4 waves per SIMD (forcing 5 spills: measured 223 -> 338 us on union3@1e-7); with the
// gradient ~140 VGPRs, 3 waves.  (Sharing one fetch between the points of a group that land in the same leaf, as
// query_kernel does, measured slower here on grids and sorted points alike: this kernel is latency-, not traffic-bound.
// Evaluating every lane of a mixed wave with the degree-3 code over zero-padded rows -- one pass instead of the
// degree-2 and degree-3 passes -- is bit-identical but needs whole lines for degree-2 leaves: 229 -> 247 us.)
template <int TOPD, bool DEFER>
__global__ __launch_bounds__(256) void query_general_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                               const double* __restrict__ xyz, size_t n,
                                                               double* __restrict__ out, uint32_t tilesPerWg,
                                                               uint32_t* __restrict__ deferCount,
                                                               uint32_t* __restrict__ deferIdx) {
    queryGeneralBody<TOPD, DEFER, false, 4, false>(t, T, xyz, n, out, nullptr, tilesPerWg, deferCount, deferIdx);
}
// depth-4 top level: 16 waves per workgroup, thin table in LDS
template <bool DEFER, int LAB = 0, int DEEP = 0>
__global__ __launch_bounds__(1024) void query_general_lds_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                                 const double* __restrict__ xyz, size_t n,
                                                                 double* __restrict__ out, uint32_t tilesPerWg,
                                                                 uint32_t* __restrict__ deferCount,
                                                                 uint32_t* __restrict__ deferIdx) {
    queryGeneralBody<4, DEFER, false, 16, true, LAB, DEEP>(t, T, xyz, n, out, nullptr, tilesPerWg, deferCount, deferIdx);
}
template <int TOPD, bool DEFER, int LAB = 0>
__global__ __launch_bounds__(256, 3) void query_general_grad_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                                    const double* __restrict__ xyz, size_t n,
                                                                    double* __restrict__ out, double* __restrict__ grad,
                                                                    uint32_t tilesPerWg, uint32_t* __restrict__ deferCount,
                                                                    uint32_t* __restrict__ deferIdx) {
    queryGeneralBody<TOPD, DEFER, true, 4, false, LAB>(t, T, xyz, n, out, grad, tilesPerWg, deferCount, deferIdx);
}

// Exclusive scan of the per-workgroup deferred counts (nWg <= 8192): offsets[b] = points deferred by workgroups
// < b, offsets[nWg] = their total.  One workgroup of 1024 threads, eight counts each.
__global__ __launch_bounds__(1024) void defer_scan_kernel(const uint32_t* __restrict__ counts, uint32_t nWg,
                                                          uint32_t* __restrict__ offsets) {
    __shared__ uint32_t sSum[1024];
    const uint32_t tid = threadIdx.x;
    uint32_t local[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t b = tid * 8 + k;
        local[k] = b < nWg ? counts[b] : 0u;
        sum += local[k];
    }
    sSum[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
        const uint32_t v = tid >= d ? sSum[tid - d] : 0u;
        __syncthreads();
        sSum[tid] += v;
        __syncthreads();
    }
    uint32_t run = sSum[tid] - sum;  // exclusive prefix of this thread's eight
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t b = tid * 8 + k;
        if (b < nWg) offsets[b] = run;
        run += local[k];
    }
    if (tid == 1023) offsets[nWg] = sSum[1023];
}

// j-th deferred point overall -> its index: the workgroup whose run holds it (binary search in the scanned counts),
// then the slot inside that run.
__device__ __forceinline__ size_t deferredPoint(uint32_t j, const uint32_t* __restrict__ offsets, uint32_t nWg,
                                                uint32_t tilesPerWg, const uint32_t* __restrict__ deferIdx) {
    uint32_t lo = 0, hi = nWg;  // offsets[lo] <= j < offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= j)
            lo = mid;
        else
            hi = mid;
    }
    return deferIdx[(size_t)lo * tilesPerWg * 256 + (j - offsets[lo])];
}

// Second pass of Query for the points query_general_kernel deferred (leaves of degree > 3), one lane each, dense
// over the concatenation of the per-workgroup lists.
template <int MAXP>
__global__ __launch_bounds__(256) void query_deep_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                         const double* __restrict__ xyz, double* __restrict__ out,
                                                         uint32_t tilesPerWg, uint32_t nWg,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ deferIdx) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    const uint32_t total = offsets[nWg];
    if ((uint32_t)(blockIdx.x * blockDim.x) >= total) return;  // workgroup-uniform
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
        const size_t i = deferredPoint(j, offsets, nWg, tilesPerWg, deferIdx);
        out[i] = queryPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], sNl, sRec);
    }
}

// Query for a handful of points (what Octree::Query(pt) sends: n = 1): one lane per point, any tree, ONE launch -- the
// batched kernels' tile machinery and, for trees with leaves of degree > 3, their scan + second pass are three more
// launches that a scalar call would pay for nothing.  Same queryPoint as the deferred pass: same values.
template <int MAXP>
__global__ __launch_bounds__(64) void query_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                       uint32_t n, double* __restrict__ out) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = queryPoint<MAXP>(t, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], sNl, sRec);
}

// Octree::QueryWithGradient + FApproxWithGradient (Octree.cpp:749-789, 904-985) for point i, any degree, one lane
__device__ void queryPointWithGradient(const TreeDev& t, size_t i, const double* __restrict__ xyz, double* __restrict__ out,
                                       double* __restrict__ grad, const double* sNl, const double* sRec) {
    const double p[3] = {(xyz[3 * i] - t.rootCentre[0]) * t.rootInvSizes[0],
                         (xyz[3 * i + 1] - t.rootCentre[1]) * t.rootInvSizes[1],
                         (xyz[3 * i + 2] - t.rootCentre[2]) * t.rootInvSizes[2]};
    const float fx = (float)p[0], fy = (float)p[1], fz = (float)p[2];
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) {
        out[i] = DBL_MAX;
        return;
    }
    double c[3] = {0.0, 0.0, 0.0}, q = 0.25;
    int depth = 0;
    NodeRec rec = t.nodes[0];
    while (rec.b == kInteriorTag) {
        uint32_t idx = rec.a;
        for (int a = 0; a < 3; ++a) {
            const bool up = p[a] >= c[a];
            idx += up ? (1u << a) : 0u;
            c[a] = up ? c[a] + q : c[a] - q;
        }
        q = q * 0.5;
        ++depth;
        rec = t.nodes[idx];
    }
    const int degree = (int)rec.b;
    const double* __restrict__ co = t.coeffs + rec.a;
    const double eps = 0.0001, s = (double)(2 << depth);
    double L[13][3][3];
    for (int a = 0; a < 3; ++a) {
        const double u = (p[a] - c[a]) * s;  // :907
        L[0][a][0] = L[0][a][1] = L[0][a][2] = sNl[depth];
        double a2 = 0.0, a1 = 1.0, b2 = 0.0, b1 = 1.0, c2 = 0.0, c1 = 1.0;
        for (int j = 1; j <= degree; ++j) {
            const double r0 = sRec[2 * j], r1 = sRec[2 * j + 1], nl = sNl[j * 11 + depth];
            const double a0 = r0 * u * a1 - r1 * a2;          // :937
            const double b0 = r0 * (u + eps) * b1 - r1 * b2;  // :941
            const double c0 = r0 * (u - eps) * c1 - r1 * c2;  // :945
            a2 = a1, a1 = a0, b2 = b1, b1 = b0, c2 = c1, c1 = c0;
            L[j][a][0] = a0 * nl, L[j][a][1] = b0 * nl, L[j][a][2] = c0 * nl;
        }
    }
    const int nc = coeffCount(degree);
    double g[3];
    for (int k = 0; k < 3; ++k) {  // :956-968
        double p1 = 0.0, m1 = 0.0;
        for (int r = 0; r < nc; ++r) {
            p1 = p1 + co[r] * L[kBasis.v[r][k]][k][1];
            m1 = m1 + co[r] * L[kBasis.v[r][k]][k][2];
        }
        g[k] = (p1 - m1) / (2.0 * eps);
    }
    const double z = t.leftAssoc ? sum3<true>(g[0] * g[0], g[1] * g[1], g[2] * g[2]) : sum3<false>(g[0] * g[0], g[1] * g[1], g[2] * g[2]);  // Eigen normalize()
    if (z > 0.0) {
        const double nrm = sqrt(z);
        g[0] = g[0] / nrm, g[1] = g[1] / nrm, g[2] = g[2] / nrm;
    }
    double f = 0.0;  // :972-984
    for (int r = 0; r < nc; ++r) {
        double lp = L[kBasis.v[r][0]][0][0];
        lp = lp * L[kBasis.v[r][1]][1][0];
        lp = lp * L[kBasis.v[r][2]][2][0];
        f = f + co[r] * lp;
    }
    out[i] = f;
    grad[3 * i] = g[0], grad[3 * i + 1] = g[1], grad[3 * i + 2] = g[2];
}

// QueryWithGradient for a handful of points in one launch (the scalar call of the drop-in), like query_few_kernel
__global__ __launch_bounds__(64) void query_grad_few_kernel(TreeDev t, const DeviceTables* __restrict__ T, const double* __restrict__ xyz,
                                                            uint32_t n, double* __restrict__ out, double* __restrict__ grad) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) queryPointWithGradient(t, i, xyz, out, grad, sNl, sRec);
}

// Octree::QueryWithGradient + FApproxWithGradient (Octree.cpp:749-789, 904-985), any degree, one lane per point:
// QueryWithGradient for one point whose leaf has degree 4 or 5, with the degree at compile time: the walk of queryPointWithGradient,
// then the leaf's coefficients into registers and evalLeafGradVals<P> -- the statements of the any-degree loop above, unrolled, its
// tables of basis values in registers instead of 936 bytes of scratch indexed through kBasis (the dense pass over union3 @ 1e-7's
// deferred points: 64 -> 20 us).  Any other degree goes through the any-degree code.
template <int P>
__device__ __forceinline__ void leafGradFixed(const TreeDev& t, const double* __restrict__ co, const double (&u)[3], int depth, size_t i,
                                              double* __restrict__ out, double* __restrict__ grad, const double* sNl, const double* sRec) {
    constexpr int N = coeffCount(P);
    double cv[N];
#pragma unroll
    for (int r = 0; r < N; ++r) cv[r] = co[r];
    double g[3];
    out[i] = evalLeafGradVals<P>(cv, u, depth, sNl, sRec, g, t.leftAssoc);
    grad[3 * i] = g[0], grad[3 * i + 1] = g[1], grad[3 * i + 2] = g[2];
}
__device__ __forceinline__ void queryPointWithGradient45(const TreeDev& t, size_t i, const double* __restrict__ xyz, double* __restrict__ out,
                                                         double* __restrict__ grad, const double* sNl, const double* sRec) {
    const double p[3] = {(xyz[3 * i] - t.rootCentre[0]) * t.rootInvSizes[0], (xyz[3 * i + 1] - t.rootCentre[1]) * t.rootInvSizes[1],
                         (xyz[3 * i + 2] - t.rootCentre[2]) * t.rootInvSizes[2]};
    const float fx = (float)p[0], fy = (float)p[1], fz = (float)p[2];
    if (!(fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f)) {
        out[i] = DBL_MAX;
        return;
    }
    double c[3] = {0.0, 0.0, 0.0}, q = 0.25;
    int depth = 0;
    NodeRec rec = t.nodes[0];
    while (rec.b == kInteriorTag) {  // :674-701
        uint32_t idx = rec.a;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const bool up = p[a] >= c[a];
            idx += up ? (1u << a) : 0u;
            c[a] = up ? c[a] + q : c[a] - q;
        }
        q = q * 0.5;
        ++depth;
        rec = t.nodes[idx];
    }
    const double s = (double)(2 << depth);
    const double u[3] = {(p[0] - c[0]) * s, (p[1] - c[1]) * s, (p[2] - c[2]) * s};  // :907
    if (rec.b == 4u)
        leafGradFixed<4>(t, t.coeffs + rec.a, u, depth, i, out, grad, sNl, sRec);
    else if (rec.b == 5u)
        leafGradFixed<5>(t, t.coeffs + rec.a, u, depth, i, out, grad, sNl, sRec);
    else
        queryPointWithGradient(t, i, xyz, out, grad, sNl, sRec);
}

// the second pass of the gradient query for the points query_general_kernel<.., GRAD> deferred (leaves of degree > 3).
// Dense over the concatenation of the per-workgroup lists, like query_deep_kernel.  FIXED45: the tree's degrees stop at 5.
template <bool FIXED45>
__global__ __launch_bounds__(256) void query_grad_deep_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                              const double* __restrict__ xyz, double* __restrict__ out,
                                                              double* __restrict__ grad, uint32_t tilesPerWg, uint32_t nWg,
                                                              const uint32_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ deferIdx) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    const uint32_t total = offsets[nWg];
    if ((uint32_t)(blockIdx.x * blockDim.x) >= total) return;  // workgroup-uniform
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    for (uint32_t jj = blockIdx.x * blockDim.x + threadIdx.x; jj < total; jj += gridDim.x * blockDim.x) {
        const size_t i = deferredPoint(jj, offsets, nWg, tilesPerWg, deferIdx);
        if constexpr (FIXED45)
            queryPointWithGradient45(t, i, xyz, out, grad, sNl, sRec);
        else
            queryPointWithGradient(t, i, xyz, out, grad, sNl, sRec);
    }
}

// Octree::QueryRay (Octree.cpp:705-746) over Ray / Ray::IntersectAABB (Source/HP/Ray.cpp:5-68): sphere tracing,
// at most 200 Query steps per ray, one lane per ray.  The reference's behaviour is kept statement by statement,
// including what looks unintended: the origin is mapped to the unit cube but the direction is not (:711); for an
// origin outside the root `intMin` is what IntersectAABB leaves in its first output -- the entry parameter in x,
// per-axis slab parameters in y and z -- not a point (:717); Query maps its argument through the root transform
// again (:726 -> :665); and on a hit t_ receives the field value (:730).  t of a miss is left untouched.
template <int MAXP>
__global__ __launch_bounds__(256) void query_ray_kernel(TreeDev t, const DeviceTables* __restrict__ T,
                                                        const double* __restrict__ origins,
                                                        const double* __restrict__ dirs, const double* __restrict__ tMax,
                                                        size_t n, uint8_t* __restrict__ hit, double* __restrict__ tOut) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double o[3], d[3], inv[3];
        int sgn[3];
        for (int a = 0; a < 3; ++a) {
            o[a] = (origins[3 * i + a] - t.rootCentre[a]) * t.rootInvSizes[a];  // :711
            d[a] = dirs[3 * i + a];
            inv[a] = 1.0 / d[a];  // Ray.cpp:10 cwiseInverse
            sgn[a] = inv[a] < 0.0 ? 1 : 0;
        }
        double im[3] = {o[0], o[1], o[2]};  // intMin
        const float fx = (float)o[0], fy = (float)o[1], fz = (float)o[2];
        const bool inside = fx >= -0.5f && fx <= 0.5f && fy >= -0.5f && fy <= 0.5f && fz >= -0.5f && fz <= 0.5f;
        bool miss = false;
        if (!inside) {  // Ray::IntersectAABB on [-0.5,0.5]^3, Ray.cpp:18-68
            double a0 = ((sgn[0] ? 0.5 : -0.5) - o[0]) * inv[0], b0 = ((sgn[0] ? -0.5 : 0.5) - o[0]) * inv[0];
            const double a1 = ((sgn[1] ? 0.5 : -0.5) - o[1]) * inv[1], b1 = ((sgn[1] ? -0.5 : 0.5) - o[1]) * inv[1];
            if ((a0 > b1) || (a1 > b0)) {
                miss = true;
            } else {
                if (a1 > a0) a0 = a1;
                if (b1 < b0) b0 = b1;
                const double a2 = ((sgn[2] ? 0.5 : -0.5) - o[2]) * inv[2], b2 = ((sgn[2] ? -0.5 : 0.5) - o[2]) * inv[2];
                if ((a0 > b2) || (a2 > b0)) {
                    miss = true;
                } else {
                    if (a2 > a0) a0 = a2;
                    im[0] = a0, im[1] = a1, im[2] = a2;
                }
            }
        }
        uint8_t h = 0;
        if (!miss) {
            const double eps = 0.0001, minStep = 0.0001, lim = tMax[i];
            double dist = 0.0;
            for (int s = 0; s < 200; ++s) {
                const double v = queryPoint<MAXP>(t, im[0] + dist * d[0], im[1] + dist * d[1], im[2] + dist * d[2], sNl, sRec);
                if (v < eps) {
                    tOut[i] = v;  // :730
                    h = 1;
                    break;
                }
                dist = dist + (v * 0.95 + minStep);  // :736
                if (dist > lim) break;
            }
        }
        hit[i] = h;
    }
}

// Sample points of Octree::OutputFunctionSlice (Octree.cpp:1144-1170): pixel (i, j) queries
// (min.x + (f32)j*step, min.y + (f32)i*step, c), step = (max.x - min.x) / nSamples in f32.  The points then go
// through the batched Query kernels (a row of pixels is a coherent run of points).
__global__ __launch_bounds__(256) void slice_points_kernel(double c, float minX, float minY, float step, uint32_t nSamples,
                                                           double* __restrict__ xyz) {
    const size_t total = (size_t)nSamples * nSamples, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const uint32_t i = (uint32_t)(p / nSamples), j = (uint32_t)(p - (size_t)i * nSamples);
        xyz[3 * p] = (double)minX + (double)((float)j * step);
        xyz[3 * p + 1] = (double)minY + (double)((float)i * step);
        xyz[3 * p + 2] = c;
    }
}

// The lattice of hpsdf_extract_surface (surface.hip): point L = i + N0 (j + N1 k) at lo + (f64)i h per axis, generated here and sent
// through queryPoint -- the device code every batched Query path reproduces bit for bit -- so a lattice value is hpsdf_query_device's
// at that point.  Neighbouring lanes are neighbouring points (x fastest): a wave walks one or two cells' nodes and coefficient lines
// together.  8 bytes written a point, nothing read but the tree.
template <int MAXP>
__global__ __launch_bounds__(256) void lattice_query_kernel(TreeDev t, const DeviceTables* __restrict__ T, SurfaceLattice g,
                                                            double* __restrict__ out) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const uint32_t total = g.nPts;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < total; p += gridDim.x * 256u) {
        const uint32_t i = p % g.np[0], r = p / g.np[0], j = r % g.np[1], k = r / g.np[1];
        const double x = g.lo[0] + (double)i * g.h[0], y = g.lo[1] + (double)j * g.h[1], z = g.lo[2] + (double)k * g.h[2];
        out[p] = queryPoint<MAXP>(t, x, y, z, sNl, sRec);
    }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Nearness weighting, Octree.cpp:1209-1247: |mean of FApprox over 100 points of the cell| for every fit of a weighted
// build, from the full coefficient arrays fit_kernel has just written (a kernel of its own: its any-degree evaluation
// keeps tables in private memory, and inside fit_kernel that put 320 bytes of scratch on every fit launch, weighted or
// not).  The points come from a hash of (cell, sample, axis) instead of std::rand; the weight itself
// (pow / exp) is applied by the host so that it matches the CPU path bit for bit.
__global__ __launch_bounds__(kFitThreads) void fit_weight_kernel(const FitBlock* __restrict__ blocks, const FitTask* __restrict__ tasks,
                                                                 const double* __restrict__ arena, double* __restrict__ means,
                                                                 const DeviceTables* __restrict__ T, const uint32_t* __restrict__ count) {
    extern __shared__ double lds[];
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    if (count != nullptr && blockIdx.x >= *count) return;  // (the device-side frontier writes the round's block count; the grid is an upper bound)
    const FitBlock blk = blocks[blockIdx.x];
    const int tid = threadIdx.x, deg = blk.degree, depth = blk.depth, G = blk.nTasks, nc = blk.rowEnd;
    stageQueryTables(T, sNl, sRec);
    double* sCo = lds;           // [G][nc] coefficients
    double* sV = lds + G * nc;   // [G][100]
    for (int s = tid; s < G * nc; s += kFitThreads) {
        const int g = s / nc, r = s - g * nc;
        sCo[s] = arena[tasks[blk.firstTask + g].outOff + r];
    }
    __syncthreads();
    for (int s = tid; s < G * 100; s += kFitThreads) {
        const int g = s / 100, n = s - g * 100;
        const FitTask& tk = tasks[blk.firstTask + g];
        const uint64_t ka = (uint64_t)__float_as_uint(tk.bmin[0]) | ((uint64_t)__float_as_uint(tk.bmin[1]) << 32);
        const uint64_t kb = (uint64_t)__float_as_uint(tk.bmin[2]) | ((uint64_t)(unsigned)depth << 32) |
                            ((uint64_t)(unsigned)deg << 40);
        const uint64_t key = splitmix64(ka) ^ splitmix64(kb ^ 0xD1B54A32D192ED03ull);
        double u[3];
        for (int a = 0; a < 3; ++a) {
            const float r = (float)(splitmix64(key + ((uint64_t)n * 3 + (uint64_t)a) * 0x9E3779B97F4A7C15ull) >> 40) *
                            (1.0f / 16777216.0f);
            const double pt = (double)(tk.bmin[a] + (tk.bmax[a] - tk.bmin[a]) * r);  // AlignedBox3f::sample()
            const double centre = (double)((tk.bmin[a] + tk.bmax[a]) / 2.0f);        // :1021 center() in f32
            u[a] = (pt - centre) * (double)(2 << depth);                             // :862
        }
        sV[s] = evalLeafGeneric(sCo + g * nc, deg, u[0], u[1], u[2], depth, sNl, sRec);
    }
    __syncthreads();
    for (int g = tid; g < G; g += kFitThreads) {
        double fIntegral = 0.0;
        for (int n = 0; n < 100; ++n) fIntegral = fIntegral + sV[g * 100 + n];
        fIntegral = fIntegral / 100.0;
        means[tasks[blk.firstTask + g].errSlot] = fabs(fIntegral);
    }
}

// Query (dGrad == nullptr) or QueryWithGradient.  dDeferCount: 2 * kQueryMaxGrid + 1 words (counts, then their scan); dDeferIdx: n + 256 *
// kQueryMaxGrid slots (both only touched for trees with leaves of degree > 3).  n < 2^32 (the caller splits larger
// batches).
hipError_t launchQuery(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dXyz, size_t n,
                       double* dOut, double* dGrad, bool allInline, uint32_t* dDeferCount, uint32_t* dDeferIdx) {
    if (n == 0) return hipSuccess;
    if (dGrad && n <= kQueryFewPoints) {
        hipLaunchKernelGGL(query_grad_few_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, t, dTables, dXyz, (uint32_t)n, dOut,
                           dGrad);
        return hipGetLastError();
    }
    if (!dGrad && n <= kQueryFewPoints) {
        const dim3 fgrid((unsigned)((n + 63) / 64)), fblock(64);
        forMaxDegree<3, 5, 12>(t.maxDegree, [&](auto P) {
            hipLaunchKernelGGL((query_few_kernel<decltype(P)::value>), fgrid, fblock, 0, stream, t, dTables, dXyz, (uint32_t)n, dOut);
        });
        return hipGetLastError();
    }
    const dim3 grid(gridFor(n)), block(256);
    if (allInline && dGrad && std::getenv("HPSDF_QUERY_GRAD_GENERAL") == nullptr) {
        if (t.topDepth == 4)
            hipLaunchKernelGGL((query_grad_kernel<4>), grid, block, 0, stream, t, dTables, dXyz, n, dOut, dGrad);
        else
            hipLaunchKernelGGL((query_grad_kernel<0>), grid, block, 0, stream, t, dTables, dXyz, n, dOut, dGrad);
        return hipGetLastError();
    }
    if (allInline && !dGrad) {
        const char* e = std::getenv("HPSDF_QUERY_DEDUPE");  // tuning knob; default on
        const bool dedupe = !(e && e[0] == '0');
        if (t.topDepth == 4) {
            if (dedupe)
                hipLaunchKernelGGL((query_kernel<4, true>), grid, block, 0, stream, t, dXyz, n, dOut);
            else
                hipLaunchKernelGGL((query_kernel<4, false>), grid, block, 0, stream, t, dXyz, n, dOut);
        } else {
            if (dedupe)
                hipLaunchKernelGGL((query_kernel<0, true>), grid, block, 0, stream, t, dXyz, n, dOut);
            else
                hipLaunchKernelGGL((query_kernel<0, false>), grid, block, 0, stream, t, dXyz, n, dOut);
        }
        return hipGetLastError();
    }
    bool defer = t.maxDegree > 3;
    const bool big = !dGrad && t.topDepth == 4 && std::getenv("HPSDF_QUERY_NO_LDSTOP") == nullptr;
    const unsigned tile = big ? 1024u : 256u;
    const size_t nTiles = (n + tile - 1) / tile;
    // The 16-wave workgroups stage the 32 KB thin table (and the basis tables) into LDS before their first tile: with 2048 of them -- eight
    // generations on 256 CUs, five tiles each -- that start was a tenth of the kernel (207 -> 194 us for 10 M points on union3 @ 1e-7 with
    // one workgroup a CU, 39 tiles each).  HPSDF_QUERY_GENERAL_WGS / _GRID: tuning knobs.
    static const unsigned bigWgs = [] { const char* e = std::getenv("HPSDF_QUERY_GENERAL_WGS"); return e ? (unsigned)std::max(1, std::atoi(e)) : 256u; }();
    static const unsigned smallWgs = [] { const char* e = std::getenv("HPSDF_QUERY_GENERAL_GRID"); return e ? (unsigned)std::max(1, std::min((int)kQueryMaxGrid, std::atoi(e))) : kQueryMaxGrid; }();
    const unsigned nWg = (unsigned)std::min<size_t>(nTiles, big ? bigWgs : smallWgs);
    const uint32_t tilesPerWg = (uint32_t)((nTiles + nWg - 1) / nWg);  // tiles b, b + G, ... of workgroup b
    const dim3 ggrid(nWg);
    const size_t lds = queryGeneralLdsBytes(big ? 16 : 4, big);
    if (big) {
        // > 64 KB of dynamic LDS is opt-in, per function and device
        const void* fn = defer ? (const void*)query_general_lds_kernel<true> : (const void*)query_general_lds_kernel<false>;
        const hipError_t ae = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ae != hipSuccess) return ae;
#ifdef HPSDF_QUERY_LAB_BUILD
        // lib/libhpsdf_lab.so only (build.py --lab; tools/query_general_floor.py): a link of the chain taken out (queryGeneralBody's LAB).
        // The values are then NOT the tree's, which is why the production library neither reads the variable nor holds these kernels.
        const char* labEnv = std::getenv("HPSDF_QUERY_LAB");
        const int lab = labEnv && dDeferCount && dDeferIdx ? std::atoi(labEnv) : 0;  // (the LAB kernels are DEFER instantiations: they need the lists)
#else
        constexpr int lab = 0;
#endif
        if (lab >= 1 && lab <= 4) {
#ifdef HPSDF_QUERY_LAB_BUILD
            const void* lf = lab == 1 ? (const void*)query_general_lds_kernel<true, 1> : lab == 2 ? (const void*)query_general_lds_kernel<true, 2>
                           : lab == 3 ? (const void*)query_general_lds_kernel<true, 3> : (const void*)query_general_lds_kernel<true, 4>;
            const hipError_t le = hipFuncSetAttribute(lf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (le != hipSuccess) return le;
            switch (lab) {
                case 1: hipLaunchKernelGGL((query_general_lds_kernel<true, 1>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx); break;
                case 2: hipLaunchKernelGGL((query_general_lds_kernel<true, 2>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx); break;
                case 3: hipLaunchKernelGGL((query_general_lds_kernel<true, 3>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx); break;
                default: hipLaunchKernelGGL((query_general_lds_kernel<true, 4>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx); break;
            }
#endif
        } else if (defer && t.maxDegree <= 5 && std::getenv("HPSDF_QUERY_TWO_PASS") == nullptr) {
            // degrees 4 and 5 are finished by the workgroup that met them (DEEP): one launch
            const hipError_t fe = hipFuncSetAttribute((const void*)query_general_lds_kernel<true, 0, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (fe != hipSuccess) return fe;
            hipLaunchKernelGGL((query_general_lds_kernel<true, 0, 5>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx);
            defer = false;
        } else if (defer)
            hipLaunchKernelGGL((query_general_lds_kernel<true>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx);
        else
            hipLaunchKernelGGL((query_general_lds_kernel<false>), ggrid, dim3(1024), lds, stream, t, dTables, dXyz, n, dOut, tilesPerWg, dDeferCount, dDeferIdx);
    } else {
#ifdef HPSDF_QUERY_LAB_BUILD  // (lib/libhpsdf_lab.so only: the gradient kernel with a link taken out -- values NOT the tree's)
        {
            const char* labEnv = std::getenv("HPSDF_QUERY_LAB");
            const int glab = labEnv && dGrad && dDeferCount && dDeferIdx && t.topDepth == 4 ? std::atoi(labEnv) : 0;
#define HPSDF_GRAD_LAB(L) case L: hipLaunchKernelGGL((query_general_grad_kernel<4, true, L>), ggrid, block, lds, stream, t, dTables, dXyz, n, dOut, dGrad, tilesPerWg, dDeferCount, dDeferIdx); return hipGetLastError();
            switch (glab) {
                HPSDF_GRAD_LAB(1) HPSDF_GRAD_LAB(2) HPSDF_GRAD_LAB(3) HPSDF_GRAD_LAB(4) HPSDF_GRAD_LAB(5) HPSDF_GRAD_LAB(6)
                default: break;
            }
#undef HPSDF_GRAD_LAB
        }
#endif
#define HPSDF_QUERY_GENERAL(TOPD, DF)                                                                               \
    do {                                                                                                            \
        if (dGrad)                                                                                                  \
            hipLaunchKernelGGL((query_general_grad_kernel<TOPD, DF>), ggrid, block, lds, stream, t, dTables, dXyz, n, dOut, \
                               dGrad, tilesPerWg, dDeferCount, dDeferIdx);                                          \
        else                                                                                                        \
            hipLaunchKernelGGL((query_general_kernel<TOPD, DF>), ggrid, block, lds, stream, t, dTables, dXyz, n, dOut,  \
                               tilesPerWg, dDeferCount, dDeferIdx);                                                 \
    } while (0)
#define HPSDF_QUERY_GENERAL_T(TOPD)         \
    do {                                    \
        if (defer)                          \
            HPSDF_QUERY_GENERAL(TOPD, true);  \
        else                                \
            HPSDF_QUERY_GENERAL(TOPD, false); \
    } while (0)
        if (t.topDepth == 4)
            HPSDF_QUERY_GENERAL_T(4);
        else
            HPSDF_QUERY_GENERAL_T(0);
#undef HPSDF_QUERY_GENERAL_T
#undef HPSDF_QUERY_GENERAL
    }
    if (defer) {
        // the per-workgroup lists are short and ragged: scan their lengths, then walk their concatenation densely
        uint32_t* dOffsets = dDeferCount + kQueryMaxGrid;
        hipLaunchKernelGGL(defer_scan_kernel, dim3(1), dim3(1024), 0, stream, dDeferCount, nWg, dOffsets);
        const dim3 dgrid(1024u);  // (grid-stride over the scanned lists: the lists' number, nWg, does not bound it)
        const uint32_t slotsPerWg = tilesPerWg * (tile / 256u);  // deferredPoint() counts in runs of 256
        if (dGrad && t.maxDegree <= 5)
            hipLaunchKernelGGL((query_grad_deep_kernel<true>), dgrid, block, 0, stream, t, dTables, dXyz, dOut, dGrad, slotsPerWg, nWg,
                               dOffsets, dDeferIdx);
        else if (dGrad)
            hipLaunchKernelGGL((query_grad_deep_kernel<false>), dgrid, block, 0, stream, t, dTables, dXyz, dOut, dGrad, slotsPerWg, nWg,
                               dOffsets, dDeferIdx);
        else if (t.maxDegree <= 5)
            hipLaunchKernelGGL((query_deep_kernel<5>), dgrid, block, 0, stream, t, dTables, dXyz, dOut, slotsPerWg, nWg, dOffsets, dDeferIdx);
        else
            hipLaunchKernelGGL((query_deep_kernel<12>), dgrid, block, 0, stream, t, dTables, dXyz, dOut, slotsPerWg, nWg, dOffsets, dDeferIdx);
    }
    return hipGetLastError();
}

hipError_t launchQueryRay(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const double* dOrigins,
                          const double* dDirs, const double* dTMax, size_t n, uint8_t* dHit, double* dT) {
    if (n == 0) return hipSuccess;
    // the evaluation code for the degrees the tree does not contain is left out (registers, no scratch)
    forMaxDegree<3, 5, 12>(t.maxDegree, [&](auto P) {
        hipLaunchKernelGGL((query_ray_kernel<decltype(P)::value>), dim3(gridFor(n)), dim3(256), 0, stream, t, dTables, dOrigins, dDirs, dTMax, n, dHit, dT);
    });
    return hipGetLastError();
}

hipError_t launchSlicePoints(hipStream_t stream, double c, float minX, float minY, float step, uint32_t nSamples,
                             double* dXyz) {
    if (nSamples == 0) return hipSuccess;
    hipLaunchKernelGGL(slice_points_kernel, dim3(gridFor((size_t)nSamples * nSamples)), dim3(256), 0, stream, c, minX, minY,
                       step, nSamples, dXyz);
    return hipGetLastError();
}

hipError_t launchQueryLattice(hipStream_t stream, const TreeDev& t, const DeviceTables* dTables, const SurfaceLattice& g, double* dOut) {
    if (g.nPts == 0) return hipSuccess;
    const dim3 grid(gridFor(g.nPts)), block(256);
    forMaxDegree<3, 5, 12>(t.maxDegree, [&](auto P) {
        hipLaunchKernelGGL((lattice_query_kernel<decltype(P)::value>), grid, block, 0, stream, t, dTables, g, dOut);
    });
    return hipGetLastError();
}

// weighted builds: |mean FApprox| of every fit of the blocks (full coefficient arrays at FitTask::outOff)
hipError_t launchFitWeight(hipStream_t stream, const FitBlock* dBlocks, uint32_t nBlocks, size_t ldsBytes, const FitTask* dTasks,
                           const double* dArena, double* dMeans, const DeviceTables* dTables, const uint32_t* dCount) {
    if (nBlocks == 0) return hipSuccess;
    hipLaunchKernelGGL(fit_weight_kernel, dim3(nBlocks), dim3(kFitThreads), ldsBytes, stream, dBlocks, dTasks, dArena, dMeans, dTables, dCount);
    return hipGetLastError();
}

}  // namespace hpsdf
