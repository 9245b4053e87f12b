// The bit-exact fit (Octree::FitPolynomial) as templates over the field kind: fitBlockBody, fit_kernel, fit_multi_kernel,
// field_kernel and their launchers.  Instantiated per kind by fit_analytic.hip, fit_samples.hip and fit_mesh.hip; fit.hip holds
// what does not depend on the kind and the public launchFit / launchFitMulti / launchFieldEval.  Depends on field_glue.hpp.
//
// Built with -ffp-contract=off: the reference CPU path runs on baseline x86-64
// (no FMA), so every multiply-add below is a separate v_mul_f64 / v_add_f64 and
// every sum runs in the reference's order.  That makes the GPU results
// bit-identical to the CPU restatement (oracle/), which is what keeps the
// octree topology identical (near-ties in the refinement decisions and in the
// heap order would otherwise flip on 1-ulp differences).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "field_glue.hpp"
#include "launch.hpp"

namespace hpsdf {

// ---------------------------------------------------------------------------
// fit: Octree::FitPolynomial, Octree.cpp:1007-1093
// ---------------------------------------------------------------------------
//
// One workgroup fits blk.nTasks cells of identical shape.  The reference loops
// samples (i,j,k) outermost and coefficients innermost; here each thread owns
// one (cell, coefficient row) accumulator and walks the samples in the same
// (i,j,k) order, so every coefficient is the same left-to-right sum.  The
// samples are processed in chunks of whole i-planes (as many as LDS holds):
// phase 1 evaluates F on the chunk's samples of every cell into LDS (all 256
// threads), phase 2 accumulates.  The per-term product
//   Lp = 1 * P_i0(x) * N_i0 * P_i1(y) * N_i1 * P_i2(z) * N_i2      (:1045-1050)
// is hoisted by loop level without changing its association.
//
// DEG > 0 fixes the degree at compile time (nq = 4*DEG+1): the innermost loop
// unrolls, the thread's P_i2 row lives in registers and the LDS reads of a row
// are issued together instead of one dependent read per term; DEG == 0 is the
// any-degree version (rows walked in groups of four, nq = 4p+1).

constexpr int kFitPiece = 8;  // terms of a row a degree-6..8 body forms at a time
#ifndef HPSDF_FIT_MIN_WAVES
#define HPSDF_FIT_MIN_WAVES 4  // waves per SIMD the register allocation must leave room for: <= 128 VGPRs.  Left alone the
                               // degree-2 kernel takes 240 (two waves per SIMD); held to 128 it spills 448 bytes and is 37 % faster
                               // (65 536 cells: 1.59 -> 2.18 TFLOP/s with the union3 field), degrees 4-5 gain 3-4 %
#endif

// acc += sum_k ((a1 * tk[k]) * n2) * F[k], k ascending
__device__ __forceinline__ double fitRowAny(double acc, double a1, const double* __restrict__ tk, double n2,
                                            const double* __restrict__ F, int nq) {
    int k = 0;
    for (; k + 4 <= nq; k += 4) {
        const double f0 = F[k], f1 = F[k + 1], f2 = F[k + 2], f3 = F[k + 3];
        const double t0 = tk[k], t1 = tk[k + 1], t2 = tk[k + 2], t3 = tk[k + 3];
        acc = acc + (a1 * t0 * n2) * f0;
        acc = acc + (a1 * t1 * n2) * f1;
        acc = acc + (a1 * t2 * n2) * f2;
        acc = acc + (a1 * t3 * n2) * f3;
    }
    for (; k < nq; ++k) acc = acc + (a1 * tk[k] * n2) * F[k];
    return acc;
}

// R > 1 (DEG > 0 only): a thread owns one row of R cells.  The product Lp of a sample does not depend on
// the cell (all cells of a workgroup share degree and depth), so it is formed once per sample and used
// for R accumulators: 2 + 3/R multiply/add instructions per (cell, sample, row) instead of 5.
template <int KIND, bool CSG, int DEG, int R, bool LEFT>
__device__ __forceinline__ void fitBlockBody(const FitBlock blk, const FitTask* __restrict__ tasks, double* __restrict__ arena,
                                             double* __restrict__ errs, double* __restrict__ mirror,
                                             const DeviceTables* __restrict__ T, const FieldDev& field, const RootMap& rm, double* lds) {
    static_assert(R == 1 || DEG > 0, "cell blocking needs a compile-time degree");
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ int32_t sMeshStack[kFitThreads / 64][kMeshStack];  // per-wave traversal stacks (mesh fields)
    __shared__ unsigned char sPosI[KIND == kFieldMesh ? 64 : 4], sPosJK[KIND == kFieldMesh ? 64 : 4];  // meshSampleOrder
    const int tid = threadIdx.x;
    const int deg = DEG > 0 ? DEG : (int)blk.degree;
    const int nq = 4 * deg + 1, nq2 = nq * nq, G = blk.nTasks;
    const int rowStart = blk.rowStart, rowEnd = blk.rowEnd, nrows = rowEnd - rowStart;
    const int gl = nq * (nq - 1) / 2;  // Legendre.h: rule n starts at n(n-1)/2 (:1016-1017)
    const int planes = blk.planesPerChunk;  // i-planes per chunk
    const int depth = blk.depth;            // every cell of the workgroup has this depth
    const bool split = blk.split != 0;       // the top-degree rows of a from-scratch fit (device_types.hpp): outOff addresses row 0

    double* sT = lds;               // [deg+1][nq]  LpX(p, root_q)
    double* sR = sT + (deg + 1) * nq;  // [nq] roots
    double* sW = sR + nq;           // [nq] weights
    double* sC = sW + nq;           // [G][8]  scale xyz, centre xyz, scale product, sample offset (bits)
    double* sF = sC + 8 * G;        // [G][planes][nq2] weighted samples of the current chunk

    stageQueryTables(T, sNl, sRec);
    for (int q = tid; q < nq; q += kFitThreads) {
        const double x = T->roots[gl + q];
        sR[q] = x;
        sW[q] = T->weights[gl + q];
        // Octree::LpX, :988-1004
        double m2 = 0.0, m1 = 1.0;
        sT[q] = 1.0;
        for (int i = 1; i <= deg; ++i) {
            const double l = T->rec[i][0] * x * m1 - T->rec[i][1] * m2;
            m2 = m1, m1 = l;
            sT[i * nq + q] = l;
        }
    }
    for (int g = tid; g < G; g += kFitThreads) {
        const FitTask& tk = tasks[blk.firstTask + g];
        double sc[3];
        for (int a = 0; a < 3; ++a) {
            sc[a] = (double)(tk.bmax[a] - tk.bmin[a]) * 0.5;               // :1020 sizes() in f32
            sC[8 * g + 3 + a] = (double)((tk.bmin[a] + tk.bmax[a]) / 2.0f);  // :1021 center() in f32
            sC[8 * g + a] = sc[a];
        }
        sC[8 * g + 6] = prod3<LEFT>(sc[0], sc[1], sc[2]);  // :1022 Eigen prod()
        sC[8 * g + 7] = __longlong_as_double((long long)tk.sampleOff);
    }
    __syncthreads();

    // phase-2 ownership: thread -> (cell slot, row); a slot is R consecutive cells; cells with > 256 rows
    // (any-degree kernel only) use two rows per thread
    // (two rows per thread only exist where a cell has more than 256 rows, i.e. beyond degree 9: the any-degree kernel.  Saying so
    // at compile time removes the second row's code from the degree-specialised kernels -- it was where the degree-2 kernel spilled
    // 448 bytes per lane: a fully unrolled plane of LDS reads for a branch that never runs)
    const bool wide = DEG == 0 && nrows > kFitThreads;
    const int slot = wide ? 0 : tid / nrows;
    const int g2 = slot * R;  // first cell of this thread
    const int r0 = rowStart + (wide ? tid : tid % nrows);
    const int r1 = r0 + kFitThreads;
    const bool act0 = wide ? (r0 < rowEnd) : (tid < ((G + R - 1) / R) * nrows);
    const bool act1 = wide && r1 < rowEnd;
    int i0a = 0, i1a = 0, i2a = 0, i0b = 0, i1b = 0, i2b = 0;
    double n0a = 0, n1a = 0, n2a = 0, n0b = 0, n1b = 0, n2b = 0;
    if (act0) {
        i0a = T->bidx[r0][0], i1a = T->bidx[r0][1], i2a = T->bidx[r0][2];
        n0a = sNl[i0a * 11 + depth], n1a = sNl[i1a * 11 + depth], n2a = sNl[i2a * 11 + depth];
    }
    if (act1) {
        i0b = T->bidx[r1][0], i1b = T->bidx[r1][1], i2b = T->bidx[r1][2];
        n0b = sNl[i0b * 11 + depth], n1b = sNl[i1b * 11 + depth], n2b = sNl[i2b * 11 + depth];
    }
    constexpr int NQF = DEG > 0 ? 4 * DEG + 1 : 1;
    double tkReg[NQF];  // this thread's P_i2 row (DEG > 0)
    if (DEG > 0) {
#pragma unroll
        for (int k = 0; k < NQF; ++k) tkReg[k] = sT[i2a * nq + k];
    }
    uint32_t meshHint = 0xFFFFFFFFu;  // closest triangle of this thread's previous sample (mesh fields)
    double acc[R];  // :1025
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    double acc1 = 0.0;

    const int cellStride = planes * nq2;  // doubles per cell in sF
    for (int iBase = 0; iBase < nq; iBase += planes) {
        const int np = min(planes, nq - iBase);
        // ---- phase 1: F on planes [iBase, iBase+np) of every cell (:1035-1040)
        if constexpr (KIND == kFieldMesh) {  // position -> root index by rank (roots are distinct), nq <= 49
            if (tid < nq) {
                int rank = 0;
                for (int b = 0; b < nq; ++b) rank += sR[b] < sR[tid] ? 1 : 0;
                sPosJK[rank] = (unsigned char)tid;
            }
            if (tid >= 64 && tid < 64 + np) {
                const int a = tid - 64;
                int rank = 0;
                for (int b = 0; b < np; ++b) rank += sR[iBase + b] < sR[iBase + a] ? 1 : 0;
                sPosI[rank] = (unsigned char)a;
            }
            __syncthreads();
        }
        if constexpr (KIND != kFieldMesh) {
            // A thread takes (cell, j, k) COLUMNS of the chunk and walks the chunk's planes i: the column's index arithmetic, its y and z
            // coordinates and (a . (b . c) order) the product w_j w_k are formed once per column instead of once per sample -- ~30 of a
            // sample's ~330 instructions at degree 2.  The sample's own statements are those of the sample-major loop below, so are the bits.
            const int cols = G * nq2;
            for (int c0 = 0; c0 < cols; c0 += kFitThreads) {
                const int cc = c0 + tid;
                const bool activeS = cc < cols;
                const int ccl = activeS ? cc : cols - 1;
                const int g = ccl / nq2, jk = ccl - g * nq2, j = jk / nq, k = jk - j * nq;
                const double* c = sC + 8 * g;
                const double uy = sR[j] * c[1] + c[4], uz = sR[k] * c[2] + c[5];
                const double wy = uy * rm.bounds[1] + rm.centre[1];  // Octree.cpp:327
                const double wz = uz * rm.bounds[2] + rm.centre[2];
                const double wj = sW[j], wk = sW[k], c6 = c[6];
                const uint64_t sbase = (uint64_t)__double_as_longlong(c[7]) + (uint64_t)(j * nq + k);
                for (int il = 0; il < np; ++il) {
                    const int i = iBase + il;
                    const double ux = sR[i] * c[0] + c[3];
                    const double wx = ux * rm.bounds[0] + rm.centre[0];
                    const uint64_t sidx = sbase + (uint64_t)(i * nq2);
                    const double fv = activeS ? fieldEvalWorld<KIND, CSG, LEFT>(field, wx, wy, wz, sidx, sNl, sRec, meshHint) : 0.0;
                    if (activeS) {
                        sF[g * cellStride + il * nq2 + jk] = c6 * prod3<LEFT>(sW[i], wj, wk) * fv;  // :1040
                        // a split fit (FitBlock::split): the field's value goes (back) into the sample buffer, from where
                        // fit_low_kernel computes the rows below the top degree
                        if (split) const_cast<double*>(field.samples)[sidx] = fv;
                    }
                }
            }
        } else {
            const int chunkSamples = np * nq2, total = G * chunkSamples;
            const float invChunk = 1.0f / (float)chunkSamples;
            for (int s0 = 0; s0 < total; s0 += kFitThreads) {  // every lane iterates (the mesh path works wave-wide)
                const int s = s0 + tid;
                const bool activeS = s < total;
                const int sc = activeS ? s : total - 1;
                // s -> (cell g, sample rem) without an integer division by the run-time chunk size
                int g = (int)(((float)sc + 0.5f) * invChunk);
                int rem = sc - g * chunkSamples;
                if (rem < 0) {
                    --g;
                    rem += chunkSamples;
                } else if (rem >= chunkSamples) {
                    ++g;
                    rem -= chunkSamples;
                }
                if constexpr (KIND == kFieldMesh) rem = meshSampleOrder(rem, np, nq, sPosI, sPosJK);
                const double* c = sC + 8 * g;
                const int il = rem / nq2, jk = rem - il * nq2, j = jk / nq, k = jk - j * nq, i = iBase + il;
                const double ux = sR[i] * c[0] + c[3], uy = sR[j] * c[1] + c[4], uz = sR[k] * c[2] + c[5];
                const double wx = ux * rm.bounds[0] + rm.centre[0];  // Octree.cpp:327
                const double wy = uy * rm.bounds[1] + rm.centre[1];
                const double wz = uz * rm.bounds[2] + rm.centre[2];
                const uint64_t sidx = (uint64_t)__double_as_longlong(c[7]) + (uint64_t)((i * nq + j) * nq + k);
                double fv;
                if constexpr (KIND == kFieldMesh) {
                    // SURVEY 3.4 user glue: (f64) mesh.SignedDistanceAtPt(p.cast<f32>()) -- one traversal per wave
                    const double mv = (double)meshSignedDistanceWave(field.mesh, V3{(float)wx, (float)wy, (float)wz}, activeS, meshHint,
                                                                     sMeshStack[tid >> 6]);
                    fv = activeS ? applyCsg<CSG>(field, mv, wx, wy, wz, sNl, sRec) : 0.0;
                } else {
                    fv = activeS ? fieldEvalWorld<KIND, CSG, LEFT>(field, wx, wy, wz, sidx, sNl, sRec, meshHint) : 0.0;
                }
                if (activeS) {
                    sF[g * cellStride + rem] = c[6] * prod3<LEFT>(sW[i], sW[j], sW[k]) * fv;  // :1040
                    // a split fit (FitBlock::split): the field's value goes (back) into the sample buffer, from where
                    // fit_mfma_low_kernel contracts the rows below the top degree
                    if constexpr (KIND != kFieldMesh)
                        if (split) const_cast<double*>(field.samples)[sidx] = fv;
                }
            }
        }
        __syncthreads();
        // ---- phase 2: accumulate the chunk, planes ascending (:1043-1053)
        if (act0) {
            const double* tj = sT + i1a * nq;
            const double* tk = sT + i2a * nq;
            for (int il = 0; il < np; ++il) {
                const double* F = sF + g2 * cellStride + il * nq2;
                const double a0 = sT[i0a * nq + iBase + il] * n0a;
#ifdef HPSDF_FIT_ROW_UNROLL
#pragma unroll HPSDF_FIT_ROW_UNROLL
#endif
                for (int j = 0; j < nq; ++j) {
                    const double a1 = a0 * tj[j] * n1a;
                    if constexpr (DEG > 0 && DEG <= 5) {
                        double lp[NQF];
#pragma unroll
                        for (int k = 0; k < NQF; ++k) lp[k] = a1 * tkReg[k] * n2a;
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const double* Fr = F + r * cellStride + j * nq;
                            double f[NQF];
#pragma unroll
                            for (int k = 0; k < NQF; ++k) f[k] = Fr[k];
#pragma unroll
                            for (int k = 0; k < NQF; ++k) acc[r] = acc[r] + lp[k] * f[k];
                        }
                    } else if constexpr (DEG > 5) {
                        // degrees 6..8: the thread's P_i2 row still lives in registers (25 / 29 / 33 doubles), the row of samples is
                        // taken in pieces of kFitPiece so that factors and samples in flight stay within the 128 registers the four
                        // waves a SIMD leave a lane (terms in the same order: k ascending)
                        const double* Fr = F + j * nq;
#pragma unroll
                        for (int k0 = 0; k0 < NQF; k0 += kFitPiece) {
                            double lp[kFitPiece], f[kFitPiece];
#pragma unroll
                            for (int k = 0; k < kFitPiece; ++k)
                                if (k0 + k < NQF) f[k] = Fr[k0 + k];
#pragma unroll
                            for (int k = 0; k < kFitPiece; ++k)
                                if (k0 + k < NQF) lp[k] = a1 * tkReg[k0 + k] * n2a;
#pragma unroll
                            for (int k = 0; k < kFitPiece; ++k)
                                if (k0 + k < NQF) acc[0] = acc[0] + lp[k] * f[k];
                        }
                    } else {
                        acc[0] = fitRowAny(acc[0], a1, tk, n2a, F + j * nq, nq);
                    }
                }
            }
        }
        if (act1) {
            const double* tj = sT + i1b * nq;
            const double* tk = sT + i2b * nq;
            for (int il = 0; il < np; ++il) {
                const double* F = sF + il * nq2;
                const double a0 = sT[i0b * nq + iBase + il] * n0b;
                for (int j = 0; j < nq; ++j) {
                    const double a1 = a0 * tj[j] * n1b;
                    acc1 = fitRowAny(acc1, a1, tk, n2b, F + j * nq, nq);
                }
            }
        }
        __syncthreads();
    }

    // coefficients out; the new rows are also stashed in LDS for the error sum.  Plain fits write only their
    // rows (outOff addresses row rowStart; an incremental fit, :847/:1012, leaves rows [0,rowStart) where the
    // earlier fit of the cell put them).  Weighted fits keep one full array per cell: outOff addresses row 0.
    const bool weighted = blk.weighted != 0;
    const int stashStride = weighted ? rowEnd : nrows, stashBase = weighted ? 0 : rowStart;
    const int outBase = split ? 0 : stashBase;  // (a split fit's array starts at row 0: the rows below rowStart come from the matrix cores)
    if (act0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (g2 + r < G) {
                const uint64_t at = tasks[blk.firstTask + g2 + r].outOff + (r0 - outBase);
                arena[at] = acc[r];
                // mirror (round 0 of the device-side frontier, one rank): host memory the device writes straight into -- a build that
                // stops after that round has its packed store there when the round closes, without a copy to wait for
                if (mirror != nullptr) mirror[at] = acc[r];
                sF[(g2 + r) * stashStride + (r0 - stashBase)] = acc[r];
            }
    }
    if (act1) {
        arena[tasks[blk.firstTask].outOff + (r1 - outBase)] = acc1;
        sF[r1 - stashBase] = acc1;
    }
    if (weighted && rowStart > 0) {  // carry the old rows over (:847)
        for (int s = tid; s < G * rowStart; s += kFitThreads) {
            const int g = s / rowStart, r = s - g * rowStart;
            const FitTask& tk = tasks[blk.firstTask + g];
            const double v = arena[tk.copyOff + r];
            arena[tk.outOff + r] = v;
            sF[g * stashStride + r] = v;
        }
    }
    __syncthreads();
    // :1062-1069  error = sum of squares of the rows of total degree == deg, in row order
    for (int g = tid; g < G; g += kFitThreads) {
        const int first = deg > 0 ? (int)T->count[deg - 1] : 0;
        double e = 0.0;
        for (int r = first > rowStart ? first : rowStart; r < rowEnd; ++r)
            if (T->bidx[r][3] == deg) {
                const double c = sF[g * stashStride + (r - stashBase)];
                e = e + c * c;
            }
        errs[tasks[blk.firstTask + g].errSlot] = e;
    }
}

// All the fits of a round in ONE launch (the device-side frontier, frontier.hip): the round's blocks lie degree by degree in
// one array and carry their degree, so a workgroup picks the compile-time-specialised body its block needs.  The blocks are
// handed out from the END of the array -- highest degree, longest fits first -- and workgroups of every degree share the chip
// at once, which is what the per-degree launches on side streams were for (their fork / join events cost 20-50 us a round).
// count: the round's number of blocks, written by the device; the grid is an upper bound.
template <int KIND, bool CSG, bool LEFT>
__global__ __launch_bounds__(kFitThreads, HPSDF_FIT_MIN_WAVES) void fit_multi_kernel(const FitBlock* __restrict__ blocks,
                                                                const FitTask* __restrict__ tasks, double* __restrict__ arena,
                                                                double* __restrict__ errs, const DeviceTables* __restrict__ T,
                                                                FieldDev field, RootMap rm, const uint32_t* __restrict__ count,
                                                                uint32_t countValue) {
    extern __shared__ double lds[];
    const uint32_t n = count ? *count : countValue;  // (the host scheduler knows the number, the device-side frontier writes it)
    if (blockIdx.x >= n) return;
    const FitBlock blk = blocks[n - 1u - blockIdx.x];
    switch (blk.degree) {
        case 2: fitBlockBody<KIND, CSG, 2, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 3: fitBlockBody<KIND, CSG, 3, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 4: fitBlockBody<KIND, CSG, 4, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 5: fitBlockBody<KIND, CSG, 5, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 6: fitBlockBody<KIND, CSG, 6, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 7: fitBlockBody<KIND, CSG, 7, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        case 8: fitBlockBody<KIND, CSG, 8, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
        default: fitBlockBody<KIND, CSG, 0, 1, LEFT>(blk, tasks, arena, errs, nullptr, T, field, rm, lds); break;
    }
}

// range == nullptr: workgroup b fits blocks[b] (the host sized the grid).  Otherwise the grid is an upper bound and
// workgroup b fits blocks[range[0] + b] if b < range[1]: the device-side frontier (frontier.hip) writes the round's block
// list and its per-degree ranges itself, so the host never learns how many blocks a round has before it launches the fits
// (a grid-stride loop over the range instead cost 37 more VGPRs at degree 3-4: one wave per SIMD less).
template <int KIND, bool CSG, int DEG, int R, bool LEFT>
__global__ __launch_bounds__(kFitThreads, HPSDF_FIT_MIN_WAVES) void fit_kernel(const FitBlock* __restrict__ blocks,
                                                          const FitTask* __restrict__ tasks, double* __restrict__ arena,
                                                          double* __restrict__ errs, double* __restrict__ mirror,
                                                          const DeviceTables* __restrict__ T, FieldDev field, RootMap rm,
                                                          const uint32_t* __restrict__ range) {
    extern __shared__ double lds[];
    uint32_t b = blockIdx.x;
    if (range != nullptr) {
        if (b >= range[1]) return;
        b += range[0];
    }
    fitBlockBody<KIND, CSG, DEG, R, LEFT>(blocks[b], tasks, arena, errs, mirror, T, field, rm, lds);
}

// F at arbitrary points (tests and diagnostics)
template <int KIND, bool CSG, bool LEFT>
__global__ __launch_bounds__(256) void field_kernel(FieldDev f, const DeviceTables* __restrict__ T,
                                                    const double* __restrict__ xyz, size_t n, double* __restrict__ out) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t hint = 0xFFFFFFFFu;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = fieldEvalWorld<KIND, CSG, LEFT>(f, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], i, sNl, sRec, hint);
}

template <int KIND, bool CSG, bool LEFT>
static void launchFitT(hipStream_t stream, int degree, int cellsPerThread, const FitBlock* dBlocks, uint32_t nBlocks,
                       size_t ldsBytes, const FitTask* dTasks, double* dArena, double* dErrs, double* dMeans,
                       const DeviceTables* dTables, const FieldDev& field, const RootMap& rm, const uint32_t* dRange) {
#define HPSDF_FIT_LAUNCH(D, RR)                                                                                       \
    hipLaunchKernelGGL((fit_kernel<KIND, CSG, D, RR, LEFT>), dim3(nBlocks), dim3(kFitThreads), ldsBytes, stream, dBlocks, \
                       dTasks, dArena, dErrs, dMeans, dTables, field, rm, dRange)
#define HPSDF_FIT_CASE(D)       \
    case D:                     \
        HPSDF_FIT_LAUNCH(D, 1); \
        break;
    if (cellsPerThread != 1 && cellsPerThread != 4) cellsPerThread = 1;
    switch (degree) {
        HPSDF_FIT_CASE(2)
        HPSDF_FIT_CASE(3)
        HPSDF_FIT_CASE(4)
        HPSDF_FIT_CASE(5)
        HPSDF_FIT_CASE(6)
        HPSDF_FIT_CASE(7)
        HPSDF_FIT_CASE(8)
        default:
            HPSDF_FIT_LAUNCH(0, 1);
    }
#undef HPSDF_FIT_CASE
#undef HPSDF_FIT_LAUNCH
}

// One launch per degree: `degree` selects the compile-time-specialised kernel (0 = any; the blocks then carry
// their own degree).
template <int KIND, bool CSG, bool LEFT>
static void launchFitMultiT(hipStream_t stream, const FitBlock* dBlocks, uint32_t maxBlocks, size_t ldsBytes, const FitTask* dTasks,
                            double* dArena, double* dErrs, const DeviceTables* dTables, const FieldDev& field, const RootMap& rm,
                            const uint32_t* dCount) {
    hipLaunchKernelGGL((fit_multi_kernel<KIND, CSG, LEFT>), dim3(maxBlocks), dim3(kFitThreads), ldsBytes, stream, dBlocks, dTasks, dArena, dErrs,
                       dTables, field, rm, dCount, maxBlocks);
}

template <int KIND, bool CSG, bool LEFT>
static void launchFieldT(hipStream_t stream, const FieldDev& f, const DeviceTables* dTables, const double* dXyz,
                         size_t n, double* dOut) {
    hipLaunchKernelGGL((field_kernel<KIND, CSG, LEFT>), dim3(gridFor(n)), dim3(256), 0, stream, f, dTables, dXyz, n, dOut);
}

// FN<KIND, csg wrapper, reduction order>(...): the instantiation for a FieldDev of one kind
#define HPSDF_DISPATCH_FIELD_ORDER(FN, K, C, field, ...)  \
    do {                                                  \
        if ((field).leftAssoc) FN<K, C, true>(__VA_ARGS__); \
        else FN<K, C, false>(__VA_ARGS__);                \
    } while (0)
#define HPSDF_DISPATCH_FIELD(FN, K, field, ...)                                                  \
    do {                                                                                         \
        if ((field).csgOp >= 0) HPSDF_DISPATCH_FIELD_ORDER(FN, K, true, field, __VA_ARGS__);     \
        else HPSDF_DISPATCH_FIELD_ORDER(FN, K, false, field, __VA_ARGS__);                       \
    } while (0)

// The three entry points of one field kind.  fit_analytic.hip, fit_samples.hip and fit_mesh.hip each instantiate them for their
// KIND (CSG wrapper on / off x reduction order: 32 fit_kernel, 4 fit_multi_kernel, 4 field_kernel), so that the kinds compile
// side by side; launchFit, launchFitMulti and launchFieldEval (fit.hip) switch on FieldDev::kind into them.
template <int KIND>
void launchFitKind(hipStream_t stream, int degree, int cellsPerThread, const FitBlock* dBlocks, uint32_t nBlocks, size_t ldsBytes,
                   const FitTask* dTasks, double* dArena, double* dErrs, double* dMirror, const DeviceTables* dTables,
                   const FieldDev& field, const RootMap& rm, const uint32_t* dRange) {
    HPSDF_DISPATCH_FIELD(launchFitT, KIND, field, stream, degree, cellsPerThread, dBlocks, nBlocks, ldsBytes, dTasks, dArena,
                         dErrs, dMirror, dTables, field, rm, dRange);
}
template <int KIND>
void launchFitMultiKind(hipStream_t stream, const FitBlock* dBlocks, uint32_t maxBlocks, size_t ldsBytes, const FitTask* dTasks,
                        double* dArena, double* dErrs, const DeviceTables* dTables, const FieldDev& field, const RootMap& rm,
                        const uint32_t* dCount) {
    HPSDF_DISPATCH_FIELD(launchFitMultiT, KIND, field, stream, dBlocks, maxBlocks, ldsBytes, dTasks, dArena, dErrs, dTables, field, rm, dCount);
}
template <int KIND>
void launchFieldKind(hipStream_t stream, const FieldDev& f, const DeviceTables* dTables, const double* dXyz, size_t n, double* dOut) {
    HPSDF_DISPATCH_FIELD(launchFieldT, KIND, f, stream, f, dTables, dXyz, n, dOut);
}
#undef HPSDF_DISPATCH_FIELD
#undef HPSDF_DISPATCH_FIELD_ORDER

// HPSDF_FIT_KIND_UNIT(extern, K) declares the three instantiations of kind K, HPSDF_FIT_KIND_UNIT(, K) makes them (fit_<kind>.hip)
#define HPSDF_FIT_KIND_UNIT(EXTERN, K)                                                                                                 \
    EXTERN template void launchFitKind<K>(hipStream_t, int, int, const FitBlock*, uint32_t, size_t, const FitTask*, double*, double*, \
                                          double*, const DeviceTables*, const FieldDev&, const RootMap&, const uint32_t*);            \
    EXTERN template void launchFitMultiKind<K>(hipStream_t, const FitBlock*, uint32_t, size_t, const FitTask*, double*, double*,      \
                                               const DeviceTables*, const FieldDev&, const RootMap&, const uint32_t*);                \
    EXTERN template void launchFieldKind<K>(hipStream_t, const FieldDev&, const DeviceTables*, const double*, size_t, double*);
HPSDF_FIT_KIND_UNIT(extern, kFieldAnalytic)
HPSDF_FIT_KIND_UNIT(extern, kFieldSamples)
HPSDF_FIT_KIND_UNIT(extern, kFieldMesh)

}  // namespace hpsdf
