// A stand-alone caller of hpsdf_clearance_block for sanitizer runs of the host-side Clearance code (csrc/clearance.hpp,
// integrate_pair.hpp, integrate.hpp, tree_bound.hpp, clearance_host.cpp, host_query.cpp): it loads two MemoryBlocks (argv[1]: A,
// argv[2]: B) and a pose of 12 doubles (argv[3]) and prints, for a few (depth, tol, max_cells, max_leaves) at iso_a = 0, the struct and
// the cells:
//   "R tag <the struct as 14 words of 64 bits, 16 hex digits each>"
//   "C tag node depth cls i j k"       one line a final cell, in the array's order
// then calls the entry with refused arguments and with a truncated block.
// No device and no library: compile it with the host sources it needs,
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Icsrc -Iinclude tests/native/clearance_block_main.cpp csrc/clearance_host.cpp csrc/integrate_pair_host.cpp
//       csrc/host_query.cpp csrc/tables.cpp -o clearance_block_main
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

static_assert(sizeof(hpsdf_clearance) == 14 * 8, "hpsdf_clearance is 112 bytes");

static void printResult(const char* tag, const hpsdf_clearance& r, const hpsdf_integrate_cell* cells, uint64_t n) {
    unsigned long long w[14];
    std::memcpy(w, &r, sizeof w);
    std::printf("R %s", tag);
    for (int k = 0; k < 14; ++k) std::printf(" %016llx", w[k]);
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
        uint32_t depth;
        double tol;
        uint32_t maxCells, maxLeaves;
    };
    const Case cases[] = {{"a", 0, 0.0, 8, 256}, {"b", 6, 0.0, 1u << 24, 256}, {"c", 7, 0.05, 1u << 24, 2}, {"d", 7, 0.0, 64, 256}};
    for (const Case& c : cases) {
        hpsdf_clearance r, r2;
        std::memset(&r, 0, sizeof r), std::memset(&r2, 0, sizeof r2);
        hpsdf_integrate_cell* cells = nullptr;
        uint64_t n = 0;
        expect(hpsdf_clearance_block(A.data(), A.size(), B.data(), B.size(), pose, 0.0, c.depth, c.tol, c.maxCells, c.maxLeaves, &r, &cells, &n) == HPSDF_OK,
               c.tag);
        printResult(c.tag, r, cells, n);
        std::free(cells);
        expect(hpsdf_clearance_block(A.data(), A.size(), B.data(), B.size(), pose, 0.0, c.depth, c.tol, c.maxCells, c.maxLeaves, &r2, nullptr, nullptr) ==
                   HPSDF_OK,
               "no cells");
        expect(std::memcmp(&r, &r2, sizeof r) == 0, "the struct does not depend on the optional output");
    }
    // refusals write nothing
    hpsdf_clearance keep;
    std::memset(&keep, 7, sizeof keep);
    hpsdf_clearance seven = keep;
    hpsdf_integrate_cell* cells = (hpsdf_integrate_cell*)&keep;
    uint64_t n = 77;
    const double inf = 1e308 * 10.0;
    double badPose[12];
    std::memcpy(badPose, pose, sizeof pose);
    badPose[7] = inf - inf;
    auto call = [&](size_t sizeB, const double* P, double ia, uint32_t depth, double tol, uint32_t maxLeaves, hpsdf_clearance* out, uint64_t* count) {
        return hpsdf_clearance_block(A.data(), A.size(), B.data(), sizeB, P, ia, depth, tol, 4096, maxLeaves, out, &cells, count);
    };
    expect(call(B.size(), pose, inf, 4, 0.0, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "iso_a refused");
    expect(call(B.size(), badPose, 0.0, 4, 0.0, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NaN pose refused");
    expect(call(B.size(), nullptr, 0.0, 4, 0.0, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NULL pose refused");
    expect(call(B.size(), pose, 0.0, 16, 0.0, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "depth 16 refused");
    expect(call(B.size(), pose, 0.0, 4, -1e-300, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "negative tol refused");
    expect(call(B.size(), pose, 0.0, 4, inf, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "infinite tol refused");
    expect(call(B.size(), pose, 0.0, 4, inf - inf, 256, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NaN tol refused");
    expect(call(B.size(), pose, 0.0, 4, 0.0, 0, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_leaves 0 refused");
    expect(call(B.size(), pose, 0.0, 4, 0.0, 65536, &keep, &n) == HPSDF_ERR_INVALID_ARGUMENT, "max_leaves 65536 refused");
    expect(call(B.size(), pose, 0.0, 4, 0.0, 256, nullptr, &n) == HPSDF_ERR_INVALID_ARGUMENT, "NULL out refused");
    expect(call(B.size(), pose, 0.0, 4, 0.0, 256, &keep, nullptr) == HPSDF_ERR_INVALID_ARGUMENT, "one of two refused");
    expect(call(B.size() - 1, pose, 0.0, 4, 0.0, 256, &keep, &n) == HPSDF_ERR_BAD_BLOCK, "truncated block refused");
    expect(std::memcmp(&keep, &seven, sizeof keep) == 0 && cells == (hpsdf_integrate_cell*)&keep && n == 77, "a refused call writes nothing");
    std::printf(bad ? "%d checks failed\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
