// A C++ caller of the drop-in's Clearance (tests/test_gpu_clearance.py compiles it with g++ the way tests/test_cxx_dropin.py compiles
// its callers): loads two MemoryBlocks (argv[1]: A, argv[2]: B) and a pose of 12 doubles (argv[3]) and prints
//   "R tag <the struct as 14 words of 64 bits, 16 hex digits each>"
//   "C tag node depth cls i j k"       one line a final cell
// for tag "a" (A against itself, the defaults but depth 6: the identity), "b" (iso_a 0.013, depth 6, tol 1e-3, max_leaves 64, with the
// cells) and "c" (depth 7, max_cells 512, with the cells).
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

static void printResult(const char* tag, const hpsdf_clearance& r, const std::vector<hpsdf_integrate_cell>& cells) {
    unsigned long long w[14];
    std::memcpy(w, &r, sizeof w);
    std::printf("R %s", tag);
    for (int k = 0; k < 14; ++k) std::printf(" %016llx", w[k]);
    std::printf("\n");
    for (const hpsdf_integrate_cell& c : cells) std::printf("C %s %u %u %u %u %u %u\n", tag, c.node, c.depth, c.cls, c.i, c.j, c.k);
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    try {
        std::vector<unsigned char> blkA = slurp(argv[1]), blkB = slurp(argv[2]), poseBytes = slurp(argv[3]);
        if (blkA.empty() || blkB.empty() || poseBytes.size() != 12 * sizeof(double)) { std::printf("input files\n"); return 3; }
        double pose[12];
        std::memcpy(pose, poseBytes.data(), sizeof pose);
        SDF::Octree a, b;
        MemoryBlock mb;
        mb.size = blkA.size(), mb.ptr = blkA.data();
        a.FromMemoryBlock(mb);
        mb.size = blkB.size(), mb.ptr = blkB.data();
        b.FromMemoryBlock(mb);
        std::vector<hpsdf_integrate_cell> cells;
        printResult("a", a.Clearance(a, nullptr, 0.0, 6), cells);
        const hpsdf_clearance rb = a.Clearance(b, pose, 0.013, 6, 1e-3, 1u << 24, 64, &cells);
        printResult("b", rb, cells);
        const hpsdf_clearance rc = a.Clearance(b, pose, 0.0, 7, 0.0, 512, 256, &cells);
        printResult("c", rc, cells);
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
