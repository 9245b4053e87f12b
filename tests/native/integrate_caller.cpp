// A C++ caller of the drop-in's Integrate (tests/test_gpu_integrate.py compiles it with g++ the way tests/test_cxx_dropin.py compiles its
// callers): loads a MemoryBlock (argv[1]) and prints, every double as the 16 hex digits of its bits,
//   "R tag status levels inside outside undecided evaluations  <24 doubles in the struct's order>"
//   "C tag node depth cls i j k"       one line a final cell
// for tag "a" (the defaults), "b" (iso 0.013, depth 6, 4 samples, with the cells) and "c" (depth 7, max_cells 512, with the cells).
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
    if (argc < 2) return 2;
    try {
        std::vector<unsigned char> blk = slurp(argv[1]);
        if (blk.empty()) { std::printf("input files\n"); return 3; }
        SDF::Octree oct;
        MemoryBlock mb;
        mb.size = blk.size(), mb.ptr = blk.data();
        oct.FromMemoryBlock(mb);
        std::vector<hpsdf_integrate_cell> cells;
        printResult("a", oct.Integrate(), cells);
        const hpsdf_integral b = oct.Integrate(0.013, 6, 4, 1u << 24, &cells);
        printResult("b", b, cells);
        const hpsdf_integral c = oct.Integrate(0.0, 7, 2, 512, &cells);
        printResult("c", c, cells);
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
