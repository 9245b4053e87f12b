// A C++ caller of the drop-in's QueryBounds and QueryBoundsGrid (tests/test_gpu_query_bounds.py compiles it with g++ the way
// tests/test_cxx_dropin.py compiles its callers): loads a MemoryBlock (argv[1]) and boxes (argv[2]: n x 6 doubles -- min, max), prints
// every double as the 16 hex digits of its bits, one row a line:
//   "B i status leaves lo hi"   batched QueryBounds, subdiv 1, the default max_leaves
//   "F i status leaves lo hi"   the same with subdiv 4 and max_leaves 3
//   "S i status leaves lo hi"   the scalar QueryBounds on the first 40 boxes (odd i: subdiv 2)
//   "G i status leaves lo hi"   QueryBoundsGrid over 5 x 4 x 3 cells of the box argv[3] holds (6 doubles), subdiv 2
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

static void row(char tag, size_t i, int status, unsigned leaves, double lo, double hi) {
    std::printf("%c %zu %d %u %016llx %016llx\n", tag, i, status, leaves, bitsOf(lo), bitsOf(hi));
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    try {
        std::vector<unsigned char> blk = slurp(argv[1]), raw = slurp(argv[2]), area = slurp(argv[3]);
        if (blk.empty() || raw.empty() || raw.size() % 48 || area.size() != 48) { std::printf("input files\n"); return 3; }
        const size_t n = raw.size() / 48;
        std::vector<double> boxes(6 * n);
        std::memcpy(boxes.data(), raw.data(), raw.size());
        SDF::Octree oct;
        MemoryBlock mb;
        mb.size = blk.size(), mb.ptr = blk.data();
        oct.FromMemoryBlock(mb);
        std::vector<double> lo(n), hi(n);
        std::vector<uint8_t> st(n);
        std::vector<uint32_t> lv(n);
        oct.QueryBounds(boxes.data(), n, lo.data(), hi.data(), st.data(), lv.data());
        for (size_t i = 0; i < n; ++i) row('B', i, st[i], lv[i], lo[i], hi[i]);
        oct.QueryBounds(boxes.data(), n, lo.data(), hi.data(), st.data(), lv.data(), 4, 3);
        for (size_t i = 0; i < n; ++i) row('F', i, st[i], lv[i], lo[i], hi[i]);
        for (size_t i = 0; i < n && i < 40; ++i) {
            const double* b = &boxes[6 * i];
            const Eigen::AlignedBox3d box(Eigen::Vector3d(b[0], b[1], b[2]), Eigen::Vector3d(b[3], b[4], b[5]));
            double l = 7.0, h = 7.0;
            uint32_t leaves = 7;
            const int s = oct.QueryBounds(box, l, h, i % 2 == 1 ? 2 : 1, 4096, &leaves);
            row('S', i, s, leaves, l, h);
        }
        double g[6];
        std::memcpy(g, area.data(), 48);
        const Eigen::AlignedBox3f view(Eigen::Vector3f((float)g[0], (float)g[1], (float)g[2]), Eigen::Vector3f((float)g[3], (float)g[4], (float)g[5]));
        const size_t cells = 5 * 4 * 3;
        std::vector<double> glo(cells), ghi(cells);
        std::vector<uint8_t> gst(cells);
        std::vector<uint32_t> glv(cells);
        oct.QueryBoundsGrid(view, Eigen::Vector3i(5, 4, 3), glo.data(), ghi.data(), gst.data(), glv.data(), 2);
        for (size_t i = 0; i < cells; ++i) row('G', i, gst[i], glv[i], glo[i], ghi[i]);
        double l = 0.0, h = 0.0;
        const Eigen::AlignedBox3d whole(Eigen::Vector3d(g[0], g[1], g[2]), Eigen::Vector3d(g[3], g[4], g[5]));
        if (oct.QueryBounds(whole, l, h) > HPSDF_BOUNDS_NOT_FINITE) { std::printf("defaults\n"); return 4; }
        oct.QueryBounds(nullptr, 0, nullptr, nullptr, nullptr);
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
