// C ABI of include/hpsdf.h: the fit micro-benchmark -- one fit launch over a lattice of cells, timed (hpsdf_bench_fit) or read back (hpsdf_fit_cells).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>

#include "launch.hpp"
#include "runtime.hpp"

using namespace hpsdf;

extern "C" {

// ---------------------------------------------------------------------------- micro-benchmark
static int benchFit(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree, int depth, uint64_t nCells, int repeats,
                    double* msPerLaunch, double* coeffsOut, double* errsOut);
int hpsdf_bench_fit(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree, int depth,
                    uint64_t nCells, int repeats, double* msPerLaunch) {
    HPSDF_TRY
    if (!msPerLaunch) return fail(HPSDF_ERR_INVALID_ARGUMENT, "bad bench arguments");
    return benchFit(ctx, cfg, field, degree, depth, nCells, repeats, msPerLaunch, nullptr, nullptr);
    HPSDF_CATCH
}
int hpsdf_fit_cells(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree, int depth, uint64_t nCells, double* coeffs,
                    double* errs) {
    HPSDF_TRY
    if (!coeffs || !errs) return fail(HPSDF_ERR_INVALID_ARGUMENT, "null argument");
    double ms = 0.0;
    return benchFit(ctx, cfg, field, degree, depth, nCells, 1, &ms, coeffs, errs);
    HPSDF_CATCH
}
static int benchFit(hpsdf_ctx* ctx, const hpsdf_config* cfg, const hpsdf_field* field, int degree, int depth, uint64_t nCells, int repeats,
                    double* msPerLaunch, double* coeffsOut, double* errsOut) {
    if (!ctx) return fail(HPSDF_ERR_NO_DEVICE, "a device context is required");
    if (!cfg || !field || !msPerLaunch || degree < 0 || degree > kMaxDegree || depth < 0 || depth > kMaxDepth || nCells == 0 ||
        repeats < 1)
        return fail(HPSDF_ERR_INVALID_ARGUMENT, "bad bench arguments");
    if (innermost(field)->kind == kHostCallback) return fail(HPSDF_ERR_UNSUPPORTED, "bench_fit needs a device field");
    HPSDF_HIP(hipSetDevice(ctx->device));
    const Tables& T = tables();
    const uint64_t nc = T.coeffCount[degree];
    const int nrows = (int)nc;
    FitShape shape = fitShape(degree, nrows, (uint32_t)std::min<uint64_t>(nCells, 0xFFFFFFFFull), false);
    bool fast = false, split = false;
    {
        FieldDev probe;
        if (ctx->fitMode == HPSDF_FIT_FAST && makeFieldDev(ctx, field, nullptr, &probe) == HPSDF_OK && fitMfmaSupports(degree, probe)) fast = true;
        // the default: top-degree rows exact, the rows below them on the matrix cores from the samples the exact kernel leaves
        if (ctx->fitMode == HPSDF_FIT_SPLIT && fitSplitSupports(degree, ctx->splitMinDegree) && innermost(field)->kind != kHostMesh) split = true;
    }
    const uint64_t rowsTop = nc - (degree > 0 ? T.coeffCount[degree - 1] : 0);
    if (fast) shape = FitShape{kMfmaCells, 1, 1, 0};  // the matrix-core fit: one workgroup per 16-cell tile
    if (split) shape = fitShape(degree, (int)rowsTop, (uint32_t)std::min<uint64_t>(nCells, 0xFFFFFFFFull), false);
    const uint64_t nq3 = (4 * (uint64_t)degree + 1) * (4 * (uint64_t)degree + 1) * (4 * (uint64_t)degree + 1);
    const int g = shape.cells, planes = shape.planes;
    std::vector<FitTask> tasks(nCells);
    const uint64_t side = 1ull << depth;
    const float h = 1.0f / (float)side;
    for (uint64_t i = 0; i < nCells; ++i) {
        const uint64_t c = i % (side * side * side);
        const uint64_t ix = c % side, iy = (c / side) % side, iz = c / (side * side);
        FitTask& t = tasks[i];
        std::memset(&t, 0, sizeof t);
        t.bmin[0] = -0.5f + (float)ix * h, t.bmin[1] = -0.5f + (float)iy * h, t.bmin[2] = -0.5f + (float)iz * h;
        for (int a = 0; a < 3; ++a) t.bmax[a] = t.bmin[a] + h;
        t.outOff = i * nc;
        t.copyOff = ~0ull;
        t.sampleOff = i * nq3;
        t.errSlot = (uint32_t)i;
        t.depth = (uint8_t)depth;
    }
    std::vector<FitBlock> blocks;
    for (uint64_t i = 0; i < nCells; i += g) {
        FitBlock fb;
        std::memset(&fb, 0, sizeof fb);
        fb.firstTask = (uint32_t)i;
        fb.nTasks = (uint16_t)std::min<uint64_t>(g, nCells - i);
        fb.degree = (uint8_t)degree;
        fb.planesPerChunk = (uint8_t)planes;
        fb.depth = (uint8_t)depth;
        fb.rowStart = (uint16_t)(split ? nc - rowsTop : 0);
        fb.rowEnd = (uint16_t)nc;
        fb.split = split ? 1 : 0;
        blocks.push_back(fb);
    }
    DevBufs bufs;
    FitTask* dT = nullptr;
    FitBlock* dB = nullptr;
    double *dA = nullptr, *dE = nullptr, *dS = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = HPSDF_OK;
    hipError_t e = bufs.alloc((void**)&dT, tasks.size() * sizeof(FitTask));
    if (e == hipSuccess) e = bufs.alloc((void**)&dB, blocks.size() * sizeof(FitBlock));
    if (e == hipSuccess) e = bufs.alloc((void**)&dA, nCells * nc * sizeof(double));
    if (e == hipSuccess) e = bufs.alloc((void**)&dE, nCells * sizeof(double));
    if (e == hipSuccess && split) e = bufs.alloc((void**)&dS, nCells * nq3 * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(dT, tasks.data(), tasks.size() * sizeof(FitTask), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dB, blocks.data(), blocks.size() * sizeof(FitBlock), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    FieldDev fd;
    RootMap rm;
    if (e == hipSuccess) rc = makeFieldDev(ctx, field, nullptr, &fd);
    for (int a = 0; a < 3; ++a) {
        rm.bounds[a] = (double)(cfg->root_max[a] - cfg->root_min[a]);
        rm.centre[a] = (double)((cfg->root_min[a] + cfg->root_max[a]) / 2.0f);
    }
    const size_t lds = shape.ldsBytes;
    if (split) fd.samples = dS;
    if (e == hipSuccess && rc == HPSDF_OK) {
        auto launch = [&]() {
            if (fast) return launchFitMfma(ctx->stream, degree, dB, (uint32_t)blocks.size(), dT, dA, dE, ctx->dTables, fd, rm);
            hipError_t le = launchFit(ctx->stream, degree, shape.cellsPerThread, dB, (uint32_t)blocks.size(), lds, dT, dA, dE, nullptr, ctx->dTables, fd, rm);
            if (le == hipSuccess && split)
                le = launchFitMfmaLow(ctx->stream, degree, dT, nullptr, 0u, (uint32_t)nCells, 0u, dA, ctx->dTables, dS, rm, fd.leftAssoc);
            return le;
        };
        e = launch();  // warm-up
        if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
        for (int r = 0; r < repeats && e == hipSuccess; ++r) e = launch();
        if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        *msPerLaunch = (double)ms / repeats;
        if (e == hipSuccess && coeffsOut) e = hipMemcpy(coeffsOut, dA, nCells * nc * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && errsOut) e = hipMemcpy(errsOut, dE, nCells * sizeof(double), hipMemcpyDeviceToHost);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return hipFail(e, "bench_fit");
    return HPSDF_OK;
}

}  // extern "C"
