// What the device sides of Integrate (integrate.hip) and IntegratePair (integrate_pair.hip) share: the row reduction -- the header's tree
// over a workgroup's 256 rows and the kernel that applies it pass after pass -- and integrateLevels' lists on the device, which differ
// between the two calls only in the two kernels a level launches.  HIP only; each unit gets its own copy of the kernels (they are in an
// unnamed namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "dev_pool.hpp"
#include "integrate.hpp"
#include "runtime.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kIntThreads = kIntBlock;
constexpr int kRowStride = 16;  // doubles between two rows of a row array (15 used)

// v of lane t + N of the same row of 16 lanes (DPP row_shl:N); a lane whose source falls outside its row gets 0
template <int N>
__device__ __forceinline__ double rowShl(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x100 + N, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x100 + N, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// The header's tree over the workgroup's 256 rows, lane t holding row t: the sum ends in lane 0.  sRows: kIntRow x 128 doubles.
__device__ __forceinline__ void blockTree(double (&row)[kIntRow], double* sRows) {
    const uint32_t t = threadIdx.x;
    if (t >= 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) sRows[k * 128 + (t - 128u)] = row[k];
    __syncthreads();
    if (t < 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + sRows[k * 128 + t];
    __syncthreads();
    if (t >= 64u && t < 128u)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) sRows[k * 128 + (t - 64u)] = row[k];
    __syncthreads();
    if (t < 64u) {
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + sRows[k * 128 + t];
        // lane t < stride reads lane t + stride < 2 stride, which held a valid sum after the step before; what the lanes above compute
        // is never read.  Strides 32 and 16 cross rows of 16 lanes (a lane permute); 8 .. 1 stay inside row 0: DPP row shifts
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + __shfl_down(row[k], 32, 64);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + __shfl_down(row[k], 16, 64);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<8>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<4>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<2>(row[k]);
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) row[k] = row[k] + rowShl<1>(row[k]);
    }
}

// rows in[0 .. n) -> out[0 .. ceil(n / 256)): workgroup b sums rows 256 b .. 256 b + 255, zero-padded
__global__ __launch_bounds__(kIntThreads) void integrate_reduce_kernel(const double* __restrict__ in, uint32_t n, double* __restrict__ out) {
    __shared__ double sRows[kIntRow * 128];
    const uint32_t i = blockIdx.x * kIntThreads + threadIdx.x;
    double row[kIntRow];
#pragma unroll
    for (int k = 0; k < kIntRow; ++k) row[k] = i < n ? in[(size_t)i * kRowStride + k] : 0.0;
    blockTree(row, sRows);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kIntRow; ++k) out[(size_t)blockIdx.x * kRowStride + k] = row[k];
}

inline uint32_t blocksOf(uint32_t n) { return (n + kIntThreads - 1) / kIntThreads; }

// integrateLevels' lists on the device: the current list, and per level the flags, their ranks, the next list, the level's final cells and
// two row arrays; everything a level took but the next list is released when the level ends, everything when the call ends (DevPool).
// Kernels launches a level's two kernels on the stream (blocksOf(n) workgroups of kIntThreads lanes each):
//   classify(s, cur, n, level, flags, notFinite)                       the class bytes, the split flags, the not-finite word
//   contribute(s, cur, n, level, flags, ranks, next, finals, rows)     the next list, the final cells, one row per workgroup
template <class Kernels>
struct DeviceIntegrateLists {
    hpsdf_ctx* ctx;
    const Kernels& kernels;
    DevPool pool;
    IntegrateCell* cur = nullptr;
    uint32_t* flags = nullptr;
    uint32_t* ranks = nullptr;
    uint32_t* notFinite = nullptr;

    int classify(int level, uint32_t n, uint32_t* nSplit, bool* finite) {
        hipStream_t s = ctx->stream;
        SURF_ALLOC(pool, flags, (size_t)n * 4, "split flags");
        SURF_ALLOC(pool, ranks, (size_t)n * 4, "split ranks");
        if (notFinite == nullptr) {
            SURF_ALLOC(pool, notFinite, 4, "flag");
            HPSDF_HIP(hipMemsetAsync(notFinite, 0, 4, s));
        }
        kernels.classify(s, cur, n, level, flags, notFinite);
        HPSDF_HIP(hipGetLastError());
        void* tmp = nullptr;
        size_t bytes = 0;
        const uint32_t* in = flags;
        uint32_t* out = ranks;
        if (const int rc = withTemp(pool, "rocprim::exclusive_scan", "scan storage", tmp, bytes, [=](void* p, size_t& b) {
                return rocprim::exclusive_scan(p, b, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
            }))
            return rc;
        uint32_t last[3] = {0, 0, 0};  // the last rank, the last flag, the flag of a non-finite cell
        HPSDF_HIP(hipMemcpyAsync(&last[0], ranks + (n - 1), 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(&last[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipMemcpyAsync(&last[2], notFinite, 4, hipMemcpyDeviceToHost, s));
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(tmp);
        *nSplit = last[0] + last[1];
        *finite = last[2] == 0u;
        return HPSDF_OK;
    }

    int contribute(int level, uint32_t n, uint32_t nSplit, std::vector<IntegrateCell>* cells, double (&T)[kIntRow]) {
        hipStream_t s = ctx->stream;
        IntegrateCell* next = nullptr;
        IntegrateCell* finals = nullptr;
        double* rowsA = nullptr;
        double* rowsB = nullptr;
        const uint32_t nFinal = n - nSplit, nb = blocksOf(n);
        if (nSplit != 0) SURF_ALLOC(pool, next, (size_t)nSplit * 8 * sizeof(IntegrateCell), "the next list");
        if (cells != nullptr && nFinal != 0) SURF_ALLOC(pool, finals, (size_t)nFinal * sizeof(IntegrateCell), "final cells");
        SURF_ALLOC(pool, rowsA, (size_t)nb * kRowStride * sizeof(double), "rows");
        SURF_ALLOC(pool, rowsB, (size_t)blocksOf(nb) * kRowStride * sizeof(double), "rows");
        const uint32_t* r = nSplit != 0 ? ranks : nullptr;
        kernels.contribute(s, cur, n, level, flags, r, next, finals, rowsA);
        HPSDF_HIP(hipGetLastError());
        double* in = rowsA;
        double* out = rowsB;
        for (uint32_t m = nb; m > 1; m = blocksOf(m)) {  // (rowsB holds blocksOf(nb) rows, rowsA more: every pass fits)
            hipLaunchKernelGGL(integrate_reduce_kernel, dim3(blocksOf(m)), dim3(kIntThreads), 0, s, in, m, out);
            HPSDF_HIP(hipGetLastError());
            double* x = in;
            in = out, out = x;
        }
        HPSDF_HIP(hipMemcpyAsync(T, in, kIntRow * sizeof(double), hipMemcpyDeviceToHost, s));
        if (finals != nullptr) {
            const size_t at = cells->size();
            cells->resize(at + nFinal);
            HPSDF_HIP(hipMemcpyAsync(cells->data() + at, finals, (size_t)nFinal * sizeof(IntegrateCell), hipMemcpyDeviceToHost, s));
        }
        HPSDF_HIP(hipStreamSynchronize(s));
        pool.release(finals), pool.release(rowsA), pool.release(rowsB), pool.release(flags), pool.release(ranks), pool.release(cur);
        cur = next;
        return HPSDF_OK;
    }

    // The call: list 0 copied from the tree's (a call writes classes into its lists), the level loop, the struct and the cells.
    // Synchronises the context stream before it returns; frees everything it took, whatever happens.
    int run(const IntegrateCell* dLeaves, uint32_t nLeaves, const IntegrateArgs& a, const double* rootCentre, const double* rootInvSizes,
            hpsdf_integral* out, hpsdf_integrate_cell** outCells, uint64_t* outCount) {
        SURF_ALLOC(pool, cur, (size_t)nLeaves * sizeof(IntegrateCell), "list 0");
        HPSDF_HIP(hipMemcpyAsync(cur, dLeaves, (size_t)nLeaves * sizeof(IntegrateCell), hipMemcpyDeviceToDevice, ctx->stream));
        IntegrateSums S;
        const int rc = integrateLevels(*this, a, nLeaves, outCells != nullptr, S);
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);  // (nothing of this call runs on when its arrays go)
            return rc;
        }
        hpsdf_integral r;
        integrateResult(S, rootCentre, rootInvSizes, a.samples, &r);
        return integrateHandOver(S, r, out, outCells, outCount);
    }
};

}  // namespace

}  // namespace hpsdf
