// The device frontier's buffers, kept by a context between Creates (hpsdf_ctx::frontierScratch): host-only state of Create's
// driver (frontier_build.cpp), which alone includes this.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "builder.hpp"
#include "frontier_dev.hpp"
#include "runtime.hpp"

namespace hpsdf {

struct FrontierWorkspace {
    int device = -1;
    bool inUse = false;
    FrDev d{};
    FrHdr* hostHdr = nullptr;  // pinned
    uint32_t nodeCap = 0;
    uint64_t arenaCap = 0, sampleCap = 0;
    double* arena = nullptr;
    double* samples = nullptr;
    // Template of the uniformly refined tree (Octree::UniformlyRefine, :112-191) and of round 0, which is the same for
    // every build: the 4096 depth-4 cells in index order, one from-scratch degree-2 fit each, cell j's rows at arena
    // offset 10 j (index order is the depth-first order of ReallocCoeffs, so a build that stops after round 0 finds
    // its packed coefficient store already sitting at the start of the arena).
    FrTemplate tmpl{};
    hpsdf_node* tmplNodes = nullptr;
    uint32_t* tmplParent = nullptr;
    uint32_t* tmplSub = nullptr;
    uint32_t* tmplLeaves = nullptr;
    double* tmplErr = nullptr;
    uint64_t* tmplJobP = nullptr;
    FitTask* tmplTasks = nullptr;
    FitBlock* tmplBlocks = nullptr;
    size_t tmplLds = 0;
    // fr_init_kernel has run for (cleanRank, cleanWorld) and nothing since: a build that ends well leaves the workspace ready for the
    // next one (the launch runs while the host hands the block over), so a Create starts with its first fit
    bool clean = false;
    bool lastWentOn = false;  // this context's last build went on past round 0 (fr_round_kernel's flag bit 1: a guess about timing, never about results)
    int cleanRank = -1, cleanWorld = -1;
    uint32_t buildStamp = 0;
    std::vector<hpsdf_node> hostNodesAfterRound0;  // the node array of a tree that stops after round 0, serialised
    char* pinned = nullptr;                        // staging of the finished block
    double* pinnedDev = nullptr;                   // ... as the device addresses it
    size_t pinnedCap = 0;
    // weighted builds: the round's |mean FApprox| values as the device writes them, the weights as the host answers, the
    // "means are there" word pair (pinned, coherent: both sides watch them while the other writes)
    double* hostMeans = nullptr;
    double* hostWeights = nullptr;
    uint32_t* hostFlag = nullptr;
    uint32_t flagStamp = 0;
    hipError_t ensureWeighting() {
        if (hostMeans) return hipSuccess;
        const size_t n = 8 * ((size_t)kFrJobs * HPSDF_JOB_HEADER_DOUBLES + kFrStatusPad);  // (indexed like errs: up to eight ranks' parts)
        hipError_t e = hipHostMalloc((void**)&hostMeans, n * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostMalloc((void**)&hostWeights, n * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostMalloc((void**)&hostFlag, 64, hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d.means, hostMeans, 0);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d.weights, hostWeights, 0);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d.hostFlag, hostFlag, 0);
        if (e == hipSuccess) {
            std::memset(hostMeans, 0, n * sizeof(double));
            for (size_t i = 0; i < n; ++i) hostWeights[i] = 1.0;
            hostFlag[0] = hostFlag[1] = 0;
        }
        return e;
    }
    // A round's fits are one launch per degree, and none of them fills the chip (a few hundred workgroups of two per CU):
    // degrees beyond the first go to side streams and run beside it
    static constexpr int kSide = 3;
    hipStream_t side[kSide] = {nullptr, nullptr, nullptr};
    hipEvent_t forkEv = nullptr, joinEv[kSide] = {nullptr, nullptr, nullptr};

    template <typename T>
    static hipError_t grow(T** p, size_t oldCount, size_t newCount, hipStream_t s, bool keep) {
        T* np = nullptr;
        hipError_t e = hipMalloc((void**)&np, newCount * sizeof(T));
        if (e != hipSuccess) return e;
        if (*p) {
            if (keep && oldCount) e = hipMemcpyAsync(np, *p, oldCount * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            (void)hipFree(*p);
        }
        *p = np;
        return e;
    }
    // device bytes per node of capacity (ensureNodes' arrays; hpsdf_ctx_set_build_limits counts with it)
    static constexpr uint64_t kBytesPerNode = sizeof(hpsdf_node) + sizeof(uint64_t) /* qErr */ + 2 * sizeof(uint32_t) /* parent, segFirst */ +
                                              (uint64_t)kFrSegs * sizeof(uint64_t) /* segOff */ + sizeof(uint64_t) /* sub */ + 2 * sizeof(uint32_t) /* candA, candB */;
    hipError_t ensureNodes(uint32_t need, hipStream_t s) {
        if (need <= nodeCap) return hipSuccess;
        uint32_t nc = nodeCap ? nodeCap : 65536u;
        while (nc < need) nc *= 2;
        hipError_t e = grow(&d.nodes, nodeCap, nc, s, true);
        if (e == hipSuccess) e = grow(&d.qErr, nodeCap, nc, s, true);
        if (e == hipSuccess) e = grow(&d.parent, nodeCap, nc, s, true);
        if (e == hipSuccess) e = grow(&d.segOff, (size_t)nodeCap * kFrSegs, (size_t)nc * kFrSegs, s, true);
        if (e == hipSuccess) e = grow(&d.segFirst, nodeCap, nc, s, true);
        if (e == hipSuccess) e = grow(&d.sub, nodeCap, nc, s, true);
        if (e == hipSuccess) e = grow(&d.candA, nodeCap, nc, s, false);
        if (e == hipSuccess) e = grow(&d.candB, nodeCap, nc, s, false);
        if (e == hipSuccess && d.packPos) {
            e = grow(&d.packPos, 0, (size_t)nc * kFrSegs, s, false);
            if (e == hipSuccess) packPosCap = nc;
        }
        if (e == hipSuccess) nodeCap = nc, d.nodeCap = nc;
        return e;
    }
    hipError_t ensureArena(uint64_t need, uint64_t used, hipStream_t s) {
        if (need <= arenaCap) return hipSuccess;
        uint64_t nc = arenaCap ? arenaCap : (1ull << 22);
        while (nc < need) nc *= 2;
        hipError_t e = grow(&arena, used, nc, s, true);
        if (e == hipSuccess) arenaCap = nc, d.arena = arena;
        return e;
    }
    hipError_t ensureSamples(uint64_t need, hipStream_t s) {
        if (need <= sampleCap) return hipSuccess;
        const uint64_t nc = (need + (1ull << 20) - 1) & ~((1ull << 20) - 1);  // to the need (GBs at high degrees), not to a power of two
        hipError_t e = grow(&samples, 0, nc, s, false);
        if (e == hipSuccess) sampleCap = nc;
        return e;
    }
    // multi-rank: errs is [world][4096 * 9], plus owners, pack positions, round-0 share
    int ranksCap = 1;
    uint64_t packCap = 0;
    FitTask* r0Tasks = nullptr;
    FitBlock* r0Blocks = nullptr;
    uint64_t* r0JobP = nullptr;
    int r0Rank = -1, r0World = -1;  // what (rank, world, error stride, replica) the three r0 arrays were built for
    bool r0Replica = false;
    uint32_t r0ErrStride = 0;
    std::vector<FitTask> hostTmplTasks, hostR0Tasks;
    hipError_t ensureRanks(int world, hipStream_t s) {
        hipError_t e = hipSuccess;
        if (world > ranksCap) {
            e = grow(&d.errs, 0, (size_t)world * (kFrJobs * HPSDF_JOB_HEADER_DOUBLES + kFrStatusPad), s, false);
            if (e == hipSuccess) ranksCap = world;
        }
        if (e == hipSuccess && world > 1 && !d.jobOwner) {
            e = hipMalloc((void**)&d.jobOwner, kFrJobs);
            if (e == hipSuccess) e = hipMalloc((void**)&r0Tasks, kFrJobs * sizeof(FitTask));
            if (e == hipSuccess) e = hipMalloc((void**)&r0Blocks, kFrJobs * sizeof(FitBlock));
            if (e == hipSuccess) e = hipMalloc((void**)&r0JobP, kFrJobs * sizeof(uint64_t));
        }
        if (e == hipSuccess && world > 1 && packPosCap < nodeCap) {
            e = grow(&d.packPos, 0, (size_t)nodeCap * kFrSegs, s, false);
            if (e == hipSuccess) packPosCap = nodeCap;
        }
        return e;
    }
    uint32_t packPosCap = 0;
    hipError_t ensurePack(uint64_t need, hipStream_t s) {
        if (need <= packCap) return hipSuccess;
        uint64_t nc = packCap ? packCap : (1ull << 20);
        while (nc < need) nc *= 2;
        hipError_t e = grow(&d.pack, 0, nc, s, false);
        if (e == hipSuccess) packCap = nc;
        return e;
    }
    hipError_t ensurePinned(size_t need) {
        if (need <= pinnedCap) return hipSuccess;
        size_t nc = pinnedCap ? pinnedCap : (1u << 20);
        while (nc < need) nc *= 2;
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr, pinnedDev = nullptr, pinnedCap = 0;
        hipError_t e = hipHostMalloc((void**)&pinned, nc, hipHostMallocCoherent | hipHostMallocMapped);  // (round 0's fit writes it while the host may look)
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&pinnedDev, pinned, 0);
        if (e == hipSuccess) pinnedCap = nc;
        return e;
    }
    template <typename T>
    static hipError_t upload(T** dst, const std::vector<T>& v) {
        hipError_t e = hipMalloc((void**)dst, std::max<size_t>(1, v.size()) * sizeof(T));
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t init(int dev, hipStream_t s) {
        device = dev;
        hipError_t e = hipMalloc((void**)&d.hdr, sizeof(FrHdr));
        if (e == hipSuccess) e = hipMalloc((void**)&d.rnd, sizeof(FrRound));
        if (e == hipSuccess) e = hipHostMalloc((void**)&hostHdr, sizeof(FrHdr), hipHostMallocCoherent | hipHostMallocMapped);  // (the host watches it while kernels write it)
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&d.hostHdr, hostHdr, 0);
        if (e == hipSuccess) e = hipMalloc((void**)&d.taken, (kFrJobs + 64) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.wBatchIdx, kFrJobs * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.wBatchErr, kFrJobs * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&d.wJobP, kFrJobs * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.wJobH, kFrJobs * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.ops, (size_t)kFrJobs * 9 * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&d.jobRecA, kFrJobs * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.jobRecB, kFrJobs * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc((void**)&d.tasks, kFrTasks * sizeof(FitTask));
        if (e == hipSuccess) e = hipMalloc((void**)&d.blocks, kFrTasks * sizeof(FitBlock));
        if (e == hipSuccess) e = hipMalloc((void**)&d.errs, (size_t)kFrJobs * HPSDF_JOB_HEADER_DOUBLES * sizeof(double));
        if (e != hipSuccess) return e;
        d.batchIdx = d.wBatchIdx, d.batchErr = d.wBatchErr, d.jobP = d.wJobP, d.jobH = d.wJobH;
        // the uniformly refined tree, from the host scheduler's own initialisation (builderBegin): identical indices
        hpsdf_build b;
        hpsdf_config cfg;
        hpsdf_config_default(&cfg);
        cfg.thread_count = 1;
        if (builderBegin(&b, &cfg, nullptr) != HPSDF_OK) return hipErrorUnknown;
        const uint32_t nT = (uint32_t)b.nodes.size();
        std::vector<uint32_t> parent(nT, 0), leaves, sub(nT, 0);
        for (uint32_t i = 0; i < nT; ++i) {
            if (b.nodes[i].child_idx != ~0ull)
                for (unsigned c = 0; c < 8; ++c) parent[b.nodes[i].child_idx + c] = i;
            else
                leaves.push_back(i);
        }
        const uint32_t nL = (uint32_t)leaves.size();
        if (nL > kFrJobs) return hipErrorUnknown;
        for (uint32_t i = nT; i-- > 1;) {  // children have larger indices than their parents
            const uint32_t own = b.nodes[i].child_idx == ~0ull ? frCoef(2) : sub[i];
            sub[parent[i]] += own;
        }
        // round 0: class (degree 2, from scratch, depth 4), slot j = job j
        int g = 1, pl = 1;
        frShape(2, false, nL, &g, &pl);
        std::vector<FitTask> tasks(nL);
        std::vector<uint64_t> jobP(nL);
        std::vector<double> errs(nL, HPSDF_INITIAL_NODE_ERR);
        for (uint32_t j = 0; j < nL; ++j) {
            const hpsdf_node& n = b.nodes[leaves[j]];
            FitTask& t = tasks[j];
            std::memset(&t, 0, sizeof t);
            for (int a = 0; a < 3; ++a) t.bmin[a] = n.aabb_min[a], t.bmax[a] = n.aabb_max[a];
            t.outOff = (uint64_t)j * frCoef(2);
            t.copyOff = ~0ull;
            t.sampleOff = (uint64_t)j * 729;
            t.errSlot = j * HPSDF_JOB_HEADER_DOUBLES;
            t.depth = n.depth;
            t.pad[0] = 2;
            jobP[j] = t.outOff;
        }
        std::vector<FitBlock> blocks((nL + g - 1) / g);
        for (uint32_t k = 0; k < blocks.size(); ++k) {
            FitBlock& fb = blocks[k];
            std::memset(&fb, 0, sizeof fb);
            fb.firstTask = k * (uint32_t)g;
            fb.nTasks = (uint16_t)std::min<uint32_t>((uint32_t)g, nL - k * (uint32_t)g);
            fb.degree = 2;
            fb.planesPerChunk = (uint8_t)pl;
            fb.rowStart = 0, fb.rowEnd = (uint16_t)frCoef(2);
            fb.depth = b.nodes[leaves[0]].depth;
        }
        tmplLds = frLds(2, g, pl);
        hostTmplTasks = tasks;
        hostNodesAfterRound0 = b.nodes;
        for (uint32_t j = 0; j < nL; ++j) {
            hostNodesAfterRound0[leaves[j]].degree = 2;
            hostNodesAfterRound0[leaves[j]].coeffs_start = (uint64_t)j * frCoef(2);
        }
        e = upload(&tmplNodes, b.nodes);
        if (e == hipSuccess) e = upload(&tmplParent, parent);
        if (e == hipSuccess) e = upload(&tmplSub, sub);
        if (e == hipSuccess) e = upload(&tmplLeaves, leaves);
        if (e == hipSuccess) e = upload(&tmplErr, errs);
        if (e == hipSuccess) e = upload(&tmplJobP, jobP);
        if (e == hipSuccess) e = upload(&tmplTasks, tasks);
        if (e == hipSuccess) e = upload(&tmplBlocks, blocks);
        tmpl.nodes = tmplNodes, tmpl.parent = tmplParent, tmpl.sub = tmplSub;
        tmpl.nNodes = nT, tmpl.nLeaves = nL, tmpl.nTasks = nL, tmpl.nBlocks = (uint32_t)blocks.size();
        tmpl.arenaRows = (uint64_t)nL * frCoef(2), tmpl.samples = (uint64_t)nL * 729;
        for (int k = 0; k < kSide && e == hipSuccess; ++k) {
            e = hipStreamCreateWithFlags(&side[k], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&joinEv[k], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&forkEv, hipEventDisableTiming);
        if (e == hipSuccess) e = ensureNodes(65536, s);
        if (e == hipSuccess) e = ensureArena(1ull << 22, 0, s);
        if (e == hipSuccess) e = ensurePinned(4u << 20);
        return e;
    }
    ~FrontierWorkspace() {
        if (device >= 0) (void)hipSetDevice(device);
        for (void* p : {(void*)d.hdr, (void*)d.rnd, (void*)d.nodes, (void*)d.qErr, (void*)d.parent, (void*)d.segOff, (void*)d.segFirst,
                        (void*)d.sub, (void*)d.taken, (void*)d.candA, (void*)d.candB, (void*)d.wBatchIdx, (void*)d.wBatchErr, (void*)d.wJobP,
                        (void*)d.wJobH, (void*)d.ops, (void*)d.jobRecA, (void*)d.jobRecB, (void*)d.tasks, (void*)d.blocks, (void*)d.errs,
                        (void*)arena, (void*)samples, (void*)tmplNodes, (void*)tmplParent, (void*)tmplSub, (void*)tmplLeaves, (void*)tmplErr,
                        (void*)tmplJobP, (void*)tmplTasks, (void*)tmplBlocks, (void*)d.jobOwner, (void*)d.packPos, (void*)d.pack, (void*)r0Tasks,
                        (void*)r0Blocks, (void*)r0JobP})
            if (p) (void)hipFree(p);
        if (hostHdr) (void)hipHostFree(hostHdr);
        if (pinned) (void)hipHostFree(pinned);
        if (hostMeans) (void)hipHostFree(hostMeans);
        if (hostWeights) (void)hipHostFree(hostWeights);
        if (hostFlag) (void)hipHostFree(hostFlag);
        for (int k = 0; k < kSide; ++k) {
            if (side[k]) (void)hipStreamDestroy(side[k]);
            if (joinEv[k]) (void)hipEventDestroy(joinEv[k]);
        }
        if (forkEv) (void)hipEventDestroy(forkEv);
    }
};

}  // namespace hpsdf
