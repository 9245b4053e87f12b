// A stand-alone caller of hpsdf_integrate_pair_block for sanitizer runs of the host-side IntegratePair code (csrc/integrate_pair.hpp,
// integrate.hpp, tree_bound.hpp, integrate_pair_host.cpp, host_query.cpp): it loads two MemoryBlocks (argv[1]: A, argv[2]: B) and a pose
// of 12 doubles (argv[3]) and prints, for a few (op, depth, samples, max_cells, max_leaves) at iso_a = 0 and iso_b = 0.013, the struct and
// the cells, every double as the 16 hex digits of its bits:
//   "R tag status levels inside outside undecided evaluations  <24 doubles in the struct's order>"
//   "C tag node depth cls i j k"       one line a final cell, in the array's order
// then calls the entry with refused arguments and with a truncated block.
// No device and no library: compile it with the host sources it needs,
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Icsrc -Iinclude tests/native/integrate_pair_block_main.cpp csrc/integrate_pair_host.cpp csrc/host_query.cpp
//       csrc/tables.cpp -o integrate_pair_block_main
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
    if (argc < 4) return 2;
    const std::vector<unsigned char> A = slurp(argv[1]), B = slurp(argv[2]), poseBytes = slurp(argv[3]);
    if (A.empty() || B.empty() || poseBytes.size() != 12 * sizeof(double)) {
        std::printf("input files\n");
        return 3;
    }
    double pose[12];
    std::memcpy(pose, poseBytes.data(), sizeof pose);
    int bad = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) std::printf("FAILED: %s (%s)\n", what, hpsdf::gError.c_str()), ++bad;
    };
    struct Case {
        const char* tag;
        uint32_t op, depth, samples, maxCells, maxLeaves;
    };
    const Case cases[] = {{"a", 0, 0, 1, 8, 256}, {"b", 0, 6, 2, 1u << 24, 256}, {"c", 1, 5, 4, 1u << 24, 2}, {"d", 2, 7, 2, 4096, 256}};
    const double isoA = 0.0, isoB = 0.013;
    for (const Case& c : cases) {
        hpsdf_integral r, r2;
        hpsdf_integrate_cell* cells = nullptr;
        uint64_t n = 0;
        expect(hpsdf_integrate_pair_block(A.data(), A.size(), B.data(), B.size(), c.op, pose, isoA, isoB, c.depth, c.samples, c.maxCells, c.maxLeaves, &r,
                                          &cells, &n) == HPSDF_OK,
               c.tag);
        printResult(c.tag, r, cells, n);
        std::free(cells);
        expect(hpsdf_integrate_pair_block(A.data(), A.size(), B.data(), B.size(), c.op, pose, isoA, isoB, c.depth, c.samples, c.maxCells, c.maxLeaves, &r2,
                                          nullptr, nullptr) == HPSDF_OK,
               "no cells");
        expect(std::memcmp(&r, &r2, sizeof r) == 0, "the struct does not depend on the optional output");
    }
    // refusals write nothing
    hpsdf_integral keep;
    std::memset(&keep, 7, sizeof keep);
    hpsdf_integral seven = keep;
    hpsdf_integrate_cell* cells = (hpsdf_integrate_cell*)&keep;
    uint64_t n = 77;
    const double inf = 1e308 * 10.0;
    double badPose[12];
    std::memcpy(badPose, pose, sizeof pose);
    badPose[7] = inf - inf;
    auto call = [&](size_t sizeB, uint32_t op, const double* P, double ia, double ib, uint32_t depth, uint32_t maxLeaves, hpsdf_integral* out,
                    uint64_t* count) {
        return hpsdf_integrate_pair_block(A.data(), A.size(), B.data(), sizeB, op, P, ia, ib, depth, 2, 4096, maxLeaves, out, &cells, count);
    };
    expect(call(B.size(), 0, pose, inf, 0.0, 4, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "iso_a refused");
    expect(call(B.size(), 0, pose, 0.0, inf - inf, 4, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NaN iso_b refused");
    expect(call(B.size(), 3, pose, 0.0, 0.0, 4, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "op 3 refused");
    expect(call(B.size(), 0, badPose, 0.0, 0.0, 4, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NaN pose refused");
    expect(call(B.size(), 0, nullptr, 0.0, 0.0, 4, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NULL pose refused");
    expect(call(B.size(), 0, pose, 0.0, 0.0, 16, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "depth 16 refused");
    expect(call(B.size(), 0, pose, 0.0, 0.0, 4, 0, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_leaves 0 refused");
    expect(call(B.size(), 0, pose, 0.0, 0.0, 4, 65536, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_leaves 65536 refused");
    expect(call(B.size(), 0, pose, 0.0, 0.0, 4, 256, nullptr, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NULL out refused");
    expect(call(B.size(), 0, pose, 0.0, 0.0, 4, 256, &keep, nullptr) == HPSDF_ERR_INVALID_ARGUMENT, "one of two refused");
    expect(call(B.size() - 1, 0, pose, 0.0, 0.0, 4, 256, &keep, &n) == HPSDF_ERR_BAD_BLOCK, "truncated block refused");
    expect(std::memcmp(&keep, &seven, sizeof keep) == 0 && cells == (hpsdf_integrate_cell*)&keep && n == 77, "a refused call writes nothing");
    std::printf(bad ? "%d checks failed\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
