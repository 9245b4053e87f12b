// A stand-alone caller of hpsdf_integrate_block for sanitizer runs of the host-side Integrate code (csrc/integrate.hpp, tree_bound.hpp,
// host_query.cpp): it loads a MemoryBlock (argv[1]) and prints, for a few (iso, depth, samples, max_cells), the struct and the cells,
// every double as the 16 hex digits of its bits:
//   "R tag status levels inside outside undecided evaluations  <24 doubles in the struct's order>"
//   "C tag node depth cls i j k"       one line a final cell, in the array's order
// then calls the entry with refused arguments and with a truncated block.
// No device and no library: compile it with the host sources it needs,
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Icsrc -Iinclude tests/native/integrate_block_main.cpp csrc/host_query.cpp csrc/tables.cpp -o integrate_block_main
// (csrc = hp-adaptive-signed-distance-field-octree_amd/csrc).  Exit status 0 and a last line "OK" when every call did what it should.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "runtime.hpp"

namespace hpsdf {
static std::string gError;
void setError(const std::string& msg) { gError = msg; }
int fail(int code, const std::string& msg) {
    gError = msg;
    return code;
}
int reductionLeftAssoc(const hpsdf_ctx*) { return 0; }
}  // namespace hpsdf

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

static void printResult(const char* tag, const hpsdf_integral& r, const hpsdf_integrate_cell* cells, uint64_t n) {
    std::printf("R %s %u %u %llu %llu %llu %llu", tag, r.status, r.levels, (unsigned long long)r.cells_inside, (unsigned long long)r.cells_outside,
                (unsigned long long)r.cells_undecided, (unsigned long long)r.evaluations);
    const double* d = &r.unit_volume_lo;  // the 24 doubles lead the struct
    for (int k = 0; k < 24; ++k) std::printf(" %016llx", bitsOf(d[k]));
    std::printf("\n");
    for (uint64_t i = 0; i < n; ++i)
        std::printf("C %s %u %u %u %u %u %u\n", tag, cells[i].node, cells[i].depth, cells[i].cls, cells[i].i, cells[i].j, cells[i].k);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::vector<unsigned char> blk = slurp(argv[1]);
    if (blk.empty()) {
        std::printf("input files\n");
        return 3;
    }
    int bad = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) std::printf("FAILED: %s (%s)\n", what, hpsdf::gError.c_str()), ++bad;
    };
    struct Case {
        const char* tag;
        double iso;
        uint32_t depth, samples, maxCells;
    };
    const Case cases[] = {{"a", 0.0, 0, 1, 8}, {"b", 0.0, 6, 2, 1u << 24}, {"c", 0.013, 7, 4, 1u << 24}, {"d", 0.0, 8, 2, 4096}};
    for (const Case& c : cases) {
        hpsdf_integral r, r2;
        hpsdf_integrate_cell* cells = nullptr;
        uint64_t n = 0;
        expect(hpsdf_integrate_block(blk.data(), blk.size(), c.iso, c.depth, c.samples, c.maxCells, &r, &cells, &n) == HPSDF_OK, c.tag);
        printResult(c.tag, r, cells, n);
        std::free(cells);
        expect(hpsdf_integrate_block(blk.data(), blk.size(), c.iso, c.depth, c.samples, c.maxCells, &r2, nullptr, nullptr) == HPSDF_OK, "no cells");
        expect(std::memcmp(&r, &r2, sizeof r) == 0, "the struct does not depend on the optional output");
    }
    // refusals write nothing
    hpsdf_integral keep;
    std::memset(&keep, 7, sizeof keep);
    hpsdf_integral seven = keep;
    hpsdf_integrate_cell* cells = (hpsdf_integrate_cell*)&keep;
    uint64_t n = 77;
    const double inf = 1e308 * 10.0;
    expect(hpsdf_integrate_block(blk.data(), blk.size(), inf, 4, 2, 4096, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "iso refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), inf - inf, 4, 2, 4096, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NaN iso refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 16, 2, 4096, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "depth 16 refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 4, 3, 4096, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "samples 3 refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 4, 2, 7, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_cells 7 refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 4, 2, (1u << 28) + 1u, &keep, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_cells refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 4, 2, 4096, nullptr, &cells, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NULL out refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size(), 0.0, 4, 2, 4096, &keep, &cells, nullptr) == HPSDF_ERR_INVALID_ARGUMENT, "one of two refused");
    expect(hpsdf_integrate_block(blk.data(), blk.size() - 1, 0.0, 4, 2, 4096, &keep, &cells, &n) == HPSDF_ERR_BAD_BLOCK, "truncated block refused");
    expect(std::memcmp(&keep, &seven, sizeof keep) == 0 && cells == (hpsdf_integrate_cell*)&keep && n == 77, "a refused call writes nothing");
    std::printf(bad ? "%d checks failed\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
