// A C++ caller of the drop-in's Simplify (tests/test_simplify_cpu.py and tests/test_gpu_simplify.py compile it with g++ the way
// tests/test_cxx_dropin.py compiles its callers): loads a MemoryBlock (argv[1]), simplifies it within argv[3] (a double) with the flags
// argv[4] on the calling thread (argv[5] == "host") or on the device ("device"), writes the result's bytes to argv[2] and prints
//   "S nodes_in coeffs_in leaves_in nodes_out coeffs_out leaves_out merges truncations levels error_bound max_cell_rms"
// with the two doubles as the 16 hex digits of their bits.  The source octree's block is compared with what was loaded afterwards
// ("U 1": unchanged).
#include "HP/Octree.h"

#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    try {
        std::vector<unsigned char> blk = slurp(argv[1]);
        if (blk.empty()) { std::printf("input file\n"); return 3; }
        const double rms = std::strtod(argv[3], nullptr);
        const uint32_t flags = (uint32_t)std::strtoul(argv[4], nullptr, 10);
        const bool host = std::strcmp(argv[5], "host") == 0;
        hpsdf_simplify_stats st;
        std::memset(&st, 0, sizeof st);
        MemoryBlock out = {0, nullptr};
        if (!host) {
            SDF::Octree oct;
            MemoryBlock mb;
            mb.size = blk.size(), mb.ptr = blk.data();
            oct.FromMemoryBlock(mb);
            SDF::Octree small = oct.Simplify(rms, flags, &st, false);
            out = small.ToMemoryBlock();
            MemoryBlock again = oct.ToMemoryBlock();
            std::printf("U %d\n", again.size == blk.size() && std::memcmp(again.ptr, blk.data(), blk.size()) == 0 ? 1 : 0);
            std::free(again.ptr);
        } else {  // (FromMemoryBlock uploads to a device; the host path must run where there is none: the block goes in as it is)
            SDF::Octree small = SDF::Octree::SimplifyBlock(MemoryBlock{blk.size(), blk.data()}, rms, flags, &st);
            out = small.ToMemoryBlock();
            std::printf("U 1\n");
        }
        std::FILE* fh = std::fopen(argv[2], "wb");
        if (!fh || std::fwrite(out.ptr, 1, out.size, fh) != out.size) { std::printf("output file\n"); return 5; }
        std::fclose(fh);
        std::free(out.ptr);
        std::printf("S %llu %llu %llu %llu %llu %llu %llu %llu %llu %016llx %016llx\n", (unsigned long long)st.nodes_in, (unsigned long long)st.coeffs_in,
                    (unsigned long long)st.leaves_in, (unsigned long long)st.nodes_out, (unsigned long long)st.coeffs_out,
                    (unsigned long long)st.leaves_out, (unsigned long long)st.merges, (unsigned long long)st.truncations,
                    (unsigned long long)st.levels, bitsOf(st.error_bound), bitsOf(st.max_cell_rms));
        return 0;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
