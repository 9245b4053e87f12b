// A C++ caller of the drop-in's IntegratePair (tests/test_gpu_integrate_pair.py compiles it with g++ the way tests/test_cxx_dropin.py
// compiles its callers): loads two MemoryBlocks (argv[1]: A, argv[2]: B) and a pose of 12 doubles (argv[3]) and prints, every double as
// the 16 hex digits of its bits,
//   "R tag status levels inside outside undecided evaluations  <24 doubles in the struct's order>"
//   "C tag node depth cls i j k"       one line a final cell
// for tag "a" (A against itself, the defaults: the intersection under the identity), "b" (the union, iso 0.013 and 0, depth 6, 4 samples,
// max_leaves 64, with the cells) and "c" (the difference, depth 7, max_cells 512, with the cells).
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

static unsigned long long bitsOf(double v) {
    unsigned long long b;
    std::memcpy(&b, &v, 8);
    return b;
}

static void printResult(const char* tag, const hpsdf_integral& r, const std::vector<hpsdf_integrate_cell>& cells) {
    std::printf("R %s %u %u %llu %llu %llu %llu", tag, r.status, r.levels, (unsigned long long)r.cells_inside, (unsigned long long)r.cells_outside,
                (unsigned long long)r.cells_undecided, (unsigned long long)r.evaluations);
    const double* d = &r.unit_volume_lo;  // the 24 doubles lead the struct
    for (int k = 0; k < 24; ++k) std::printf(" %016llx", bitsOf(d[k]));
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
        printResult("a", a.IntegratePair(a, HPSDF_PAIR_INTERSECTION), cells);
        const hpsdf_integral rb = a.IntegratePair(b, HPSDF_PAIR_UNION, pose, 0.013, 0.0, 6, 4, 1u << 24, 64, &cells);
        printResult("b", rb, cells);
        const hpsdf_integral rc = a.IntegratePair(b, HPSDF_PAIR_DIFFERENCE, pose, 0.0, 0.0, 7, 2, 512, 256, &cells);
        printResult("c", rc, cells);
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
