// QueryBounds: a guaranteed range [lo, hi] of Query over each of n axis-aligned boxes (include/hpsdf.h, "QueryBounds"; the walk's
// statements are tree_bound.hpp's boundsWalk, the leaf evaluation is Query's evalLeaf, leaf_eval.hpp).
//
//   query_bounds_kernel<MAXP, Boxes>  any tree, one lane per box, grid-stride.  Boxes is where a lane's box comes from: rows of six
//                                     doubles (BoxArray: 48 bytes read a box) or the cells of a lattice (BoxGrid: nothing read, the
//                                     corners are lo + (double)i * h) -- one walk for both.  17 bytes written a box, 21 with the leaf
//                                     counts.  A lane walks until its box is done; lanes that are done idle until the last lane of
//                                     their wave is: a wave costs its largest box.  (No wave cooperating on one large box.)
// The walk's stack is two words per level -- the first child and the mask of children still to visit -- and lives in LDS, indexed
// [level][lane]: 12 x 256 x (4 + 1) bytes a workgroup, no bank conflicts (a wave's lanes read one row), no scratch.  The centre of the
// node a level holds is rebuilt from the path (tree_bound.hpp), so no array of doubles is indexed at run time.
// The double outputs leave through non-temporal stores like Query's; the byte and 32-bit outputs are plain stores.
//
// The leaves' constants G_x, G_y, G_z, S depend on the tree alone: hpsdf_tree::boundConsts builds them at the first bounds call on a
// tree (leaf_depth_kernel / leaf_consts_kernel, tree_bound.hpp: the sparse extraction's own kernels), under the tree's lock, and the
// tree keeps them until it is destroyed; every later call is a launch and nothing else.
//
// Built with -ffp-contract=off like every other unit: the host version (host_query.cpp, hostBoundsRows) gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "device_types.hpp"
#include "launch.hpp"
#include "leaf_eval.hpp"
#include "runtime.hpp"
#include "tree_bound.hpp"

namespace hpsdf {

namespace {

constexpr unsigned kBoundsThreads = 256;

struct BoundsOut {
    double* lo;  // never null
    double* hi;
    uint8_t* status;
    uint32_t* leaves;  // may be null
};

// boundsWalk's Stack in LDS: level d of this lane at [d * kBoundsThreads + lane]
struct LdsBoundsStack {
    uint32_t* f;
    uint8_t* m;
    __device__ __forceinline__ uint32_t first(int d) const { return f[d * kBoundsThreads]; }
    __device__ __forceinline__ uint32_t mask(int d) const { return m[d * kBoundsThreads]; }
    __device__ __forceinline__ void setFirst(int d, uint32_t v) { f[d * kBoundsThreads] = v; }
    __device__ __forceinline__ void setMask(int d, uint32_t v) { m[d * kBoundsThreads] = (uint8_t)v; }
};

}  // namespace

// Any tree, one lane per box, grid-stride in workgroups of blockDim.x <= 256 lanes.  No output array may alias the boxes.
template <int MAXP, class Boxes>
__global__ __launch_bounds__(kBoundsThreads) void query_bounds_kernel(ClsTree t, const DeviceTables* __restrict__ T, Boxes boxes, size_t n,
                                                                      uint32_t subdiv, uint32_t maxLeaves, BoundsOut o) {
    __shared__ double sNl[13 * 11];
    __shared__ double sRec[26];
    __shared__ uint32_t sFirst[kLevels * kBoundsThreads];
    __shared__ uint8_t sMask[kLevels * kBoundsThreads];
    stageQueryTables(T, sNl, sRec);
    __syncthreads();
    const DevEval<MAXP> eval{sNl, sRec};
    LdsBoundsStack st{sFirst + threadIdx.x, sMask + threadIdx.x};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double a[3], b[3];
        boxes.get(i, a, b);
        BoundsRow r;
        boundsWalk(t, a, b, subdiv, maxLeaves, eval, st, r);
        __builtin_nontemporal_store(r.lo, &o.lo[i]);
        __builtin_nontemporal_store(r.hi, &o.hi[i]);
        o.status[i] = (uint8_t)r.status;
        if (o.leaves != nullptr) o.leaves[i] = r.leaves;
    }
}

// dBoxes == nullptr: the cells of *grid.  dLo, dHi and dStatus are required, dLeaves may be null.  Every index is a size_t.
hipError_t launchQueryBounds(hipStream_t stream, const ClsTree& t, int maxDegree, const DeviceTables* dTables, const double* dBoxes,
                             const BoxGrid* grid, size_t n, uint32_t subdiv, uint32_t maxLeaves, double* dLo, double* dHi, uint8_t* dStatus,
                             uint32_t* dLeaves) {
    if (n == 0) return hipSuccess;
    const BoundsOut o{dLo, dHi, dStatus, dLeaves};
    const PointLaunch l(n);
    forMaxDegree<3, 5, 12>(maxDegree, [&](auto P) {
        constexpr int MAXP = decltype(P)::value;
        if (dBoxes != nullptr)
            hipLaunchKernelGGL((query_bounds_kernel<MAXP, BoxArray>), l.grid, l.block, 0, stream, t, dTables, BoxArray{dBoxes}, n, subdiv, maxLeaves, o);
        else
            hipLaunchKernelGGL((query_bounds_kernel<MAXP, BoxGrid>), l.grid, l.block, 0, stream, t, dTables, *grid, n, subdiv, maxLeaves, o);
    });
    return hipGetLastError();
}

}  // namespace hpsdf

using namespace hpsdf;

// The leaves' constants of this tree on its device, built once: the first caller launches the two kernels on its context's stream and
// waits for them under the lock, so whichever stream a later call runs on finds them complete.
int hpsdf_tree::boundConsts(hpsdf_ctx* ctx) const {
    if (boundReady.load(std::memory_order_acquire)) return HPSDF_OK;
    std::lock_guard<std::mutex> guard(boundLock);
    if (boundReady.load(std::memory_order_relaxed)) return HPSDF_OK;
    HPSDF_HIP(hipSetDevice(device));
    uint8_t* dDepth = nullptr;
    double* dConsts = nullptr;
    hipError_t e = hipMalloc((void**)&dDepth, nNodes < 256 ? 256 : (size_t)nNodes);
    if (e == hipSuccess) e = hipMalloc((void**)&dConsts, (size_t)nNodes * 4 * sizeof(double));
    if (e == hipSuccess) e = launchLeafConsts(ctx->stream, this, ctx->dTables, dDepth, dConsts);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (dDepth) (void)hipFree(dDepth);
    if (e != hipSuccess) {
        if (dConsts) (void)hipFree(dConsts);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            return fail(HPSDF_ERR_OUT_OF_MEMORY, "hpsdf_query_bounds: out of device memory (leaf constants)");
        }
        return hipFail(e, "leaf constants");
    }
    dBoundConsts = dConsts;
    boundReady.store(true, std::memory_order_release);
    return HPSDF_OK;
}

// their host copy, for the calls answered on the calling thread (the device's values: the same kernels' bits as the *_block entries
// compute with leafBound on the host)
int hpsdf_tree::boundHostCopies(hpsdf_ctx* ctx) const {
    if (boundHostReady.load(std::memory_order_acquire)) return HPSDF_OK;
    if (const int rc = boundConsts(ctx)) return rc;
    std::lock_guard<std::mutex> guard(boundLock);
    if (boundHostReady.load(std::memory_order_relaxed)) return HPSDF_OK;
    HPSDF_HIP(hipSetDevice(device));
    hBoundConsts.resize((size_t)nNodes * 4);
    HPSDF_HIP(hipMemcpy(hBoundConsts.data(), dBoundConsts, (size_t)nNodes * 4 * sizeof(double), hipMemcpyDeviceToHost));
    boundHostReady.store(true, std::memory_order_release);
    return HPSDF_OK;
}
