// A stand-alone caller of hpsdf_clearance_batch_block for sanitizer runs of the host-side batch code (csrc/clearance.hpp,
// clearance_host.cpp and what they use): it loads two MemoryBlocks (argv[1]: A, argv[2]: B) and n poses of 12 doubles (argv[3]) and
// prints, for a few (depth, tol, decide, max_cells, max_leaves) at iso_a = 0, one line a pose
//   "R tag<pose index> <the struct as 14 words of 64 bits, 16 hex digits each>"
// checks every struct against hpsdf_clearance_block for that pose where decide is off, then calls the entry with refused arguments.
// No device and no library: compile it with the host sources it needs,
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Icsrc -Iinclude tests/native/clearance_batch_block_main.cpp csrc/clearance_host.cpp
//       csrc/integrate_pair_host.cpp csrc/host_query.cpp csrc/tables.cpp -o clearance_batch_block_main
// (csrc = hp-adaptive-signed-distance-field-octree_amd/csrc).  Exit status 0 and a last line "OK" when every call did what it should.
#include <cmath>
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

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::vector<unsigned char> A = slurp(argv[1]), B = slurp(argv[2]), poseBytes = slurp(argv[3]);
    if (A.empty() || B.empty() || poseBytes.empty() || poseBytes.size() % (12 * sizeof(double)) != 0) {
        std::printf("input files\n");
        return 3;
    }
    const size_t n = poseBytes.size() / (12 * sizeof(double));
    std::vector<double> poses(12 * n);
    std::memcpy(poses.data(), poseBytes.data(), poseBytes.size());
    int bad = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) std::printf("FAILED: %s (%s)\n", what, hpsdf::gError.c_str()), ++bad;
    };
    const double nan = std::nan("");
    struct Case {
        const char* tag;
        uint32_t depth;
        double tol, decide;
        uint32_t maxCells, maxLeaves;
    };
    const Case cases[] = {{"a", 0, 0.0, nan, 8, 256}, {"b", 5, 0.0, nan, 1u << 24, 256}, {"c", 6, 0.05, nan, 1u << 24, 2}, {"d", 6, 0.0, nan, 64, 256},
                          {"e", 6, 0.0, 0.0, 1u << 24, 256}};
    for (const Case& c : cases) {
        std::vector<hpsdf_clearance> r(n);
        expect(hpsdf_clearance_batch_block(A.data(), A.size(), B.data(), B.size(), poses.data(), n, 0.0, c.depth, c.tol, c.decide, c.maxCells, c.maxLeaves,
                                           1u << 24, r.data()) == HPSDF_OK,
               c.tag);
        for (size_t i = 0; i < n; ++i) {
            unsigned long long w[14];
            std::memcpy(w, &r[i], sizeof w);
            std::printf("R %s%zu", c.tag, i);
            for (int k = 0; k < 14; ++k) std::printf(" %016llx", w[k]);
            std::printf("\n");
            if (c.decide == c.decide) continue;
            hpsdf_clearance one;
            expect(hpsdf_clearance_block(A.data(), A.size(), B.data(), B.size(), poses.data() + 12 * i, 0.0, c.depth, c.tol, c.maxCells, c.maxLeaves, &one,
                                         nullptr, nullptr) == HPSDF_OK,
                   "the single call");
            expect(std::memcmp(&one, &r[i], sizeof one) == 0, "a pose of the batch is the single call's struct");
        }
    }
    // refusals write nothing
    std::vector<hpsdf_clearance> keep(n);
    std::memset(keep.data(), 7, n * sizeof(hpsdf_clearance));
    const std::vector<hpsdf_clearance> seven = keep;
    const double inf = 1e308 * 10.0;
    std::vector<double> badPoses = poses;
    badPoses[12 * (n - 1) + 7] = inf;
    auto call = [&](size_t sizeB, const double* P, size_t count, double decide, uint32_t maxCells, uint32_t maxTotal, hpsdf_clearance* out) {
        return hpsdf_clearance_batch_block(A.data(), A.size(), B.data(), sizeB, P, count, 0.0, 4, 0.0, decide, maxCells, 256, maxTotal, out);
    };
    expect(call(B.size(), badPoses.data(), n, nan, 4096, 4096, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "a non-finite entry of the last pose refused");
    expect(call(B.size(), nullptr, n, nan, 4096, 4096, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "NULL poses refused");
    expect(call(B.size(), poses.data(), n, inf, 4096, 4096, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "an infinite decide refused");
    expect(call(B.size(), poses.data(), n, nan, 4096, 4095, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "max_total_cells below max_cells refused");
    expect(call(B.size(), poses.data(), n, nan, 4096, (1u << 28) + 1u, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "max_total_cells above 2^28 refused");
    expect(call(B.size(), poses.data(), ((size_t)1 << 24) + 1, nan, 4096, 4096, keep.data()) == HPSDF_ERR_INVALID_ARGUMENT, "n above 2^24 refused");
    expect(call(B.size(), poses.data(), n, nan, 4096, 4096, nullptr) == HPSDF_ERR_INVALID_ARGUMENT, "NULL out refused");
    expect(call(B.size() - 1, poses.data(), n, nan, 4096, 4096, keep.data()) == HPSDF_ERR_BAD_BLOCK, "truncated block refused");
    expect(call(B.size(), nullptr, 0, nan, 4096, 4096, nullptr) == HPSDF_OK, "n = 0 is fine without arrays");
    expect(std::memcmp(keep.data(), seven.data(), n * sizeof(hpsdf_clearance)) == 0, "a refused call writes nothing");
    std::printf(bad ? "%d checks failed\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
