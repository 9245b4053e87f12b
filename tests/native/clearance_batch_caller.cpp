// A C++ caller of the drop-in's ClearanceBatch (tests/test_gpu_clearance_batch.py compiles it with g++ the way tests/test_cxx_dropin.py
// compiles its callers): loads two MemoryBlocks (argv[1]: A, argv[2]: B) and n poses of 12 doubles each (argv[3]) and prints one line a
// pose
//   "R tag<pose index> <the struct as 14 words of 64 bits, 16 hex digits each>"
// for tag "a" (iso_a 1e-5, depth 6, the other defaults), "b" (the same with tol 1e-3, max_cells 512, max_leaves 64) and "c" (depth 6,
// decide 1e-6, max_total_cells 1 << 16).
#include "HP/Octree.h"

#include <cstdio>
#include <cstring>
#include <vector>

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> buf;
    std::FILE* fh = std::fopen(path, "rb");
    if (!fh) return buf;
    std::fseek(fh, 0, SEEK_END);
    buf.resize((size_t)std::ftell(fh));
    std::fseek(fh, 0, SEEK_SET);
    if (!buf.empty() && std::fread(buf.data(), 1, buf.size(), fh) != buf.size()) buf.clear();
    std::fclose(fh);
    return buf;
}

static_assert(sizeof(hpsdf_clearance) == 14 * 8, "hpsdf_clearance is 112 bytes");

static void printResults(const char* tag, const std::vector<hpsdf_clearance>& rs) {
    for (size_t i = 0; i < rs.size(); ++i) {
        unsigned long long w[14];
        std::memcpy(w, &rs[i], sizeof w);
        std::printf("R %s%zu", tag, i);
        for (int k = 0; k < 14; ++k) std::printf(" %016llx", w[k]);
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    try {
        std::vector<unsigned char> blkA = slurp(argv[1]), blkB = slurp(argv[2]), poseBytes = slurp(argv[3]);
        if (blkA.empty() || blkB.empty() || poseBytes.empty() || poseBytes.size() % (12 * sizeof(double)) != 0) { std::printf("input files\n"); return 3; }
        const size_t n = poseBytes.size() / (12 * sizeof(double));
        std::vector<double> poses(12 * n);
        std::memcpy(poses.data(), poseBytes.data(), poseBytes.size());
        SDF::Octree a, b;
        MemoryBlock mb;
        mb.size = blkA.size(), mb.ptr = blkA.data();
        a.FromMemoryBlock(mb);
        mb.size = blkB.size(), mb.ptr = blkB.data();
        b.FromMemoryBlock(mb);
        printResults("a", a.ClearanceBatch(b, poses.data(), n, 1e-5, 6));
        printResults("b", a.ClearanceBatch(b, poses.data(), n, 1e-5, 6, 1e-3, 512, 64));
        printResults("c", a.ClearanceBatch(b, poses.data(), n, 1e-5, 6, 0.0, 1u << 16, 256, 1e-6, 1u << 16));
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
