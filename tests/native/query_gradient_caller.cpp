// A C++ caller of the drop-in's QueryGradient (scalar and batched) and SurfaceNormals (tests/test_gpu_query_gradient.py compiles it with
// g++ the way tests/test_cxx_dropin.py compiles its callers): loads a MemoryBlock (argv[1]) and points (argv[2]: n x 3 doubles), prints
// every result as the 16 hex digits of its bits, one row a line:
//   "B i f gx gy gz"   batched QueryGradient, unit off      "U i f gx gy gz"   the same with unit_ = true
//   "S i f gx gy gz"   the scalar overload on the first 40 points
//   "N i nx ny nz"     SurfaceNormals of ExtractSurface(root box, 24^3); "V i x y z" its vertices; "M nVerts nTris"
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

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        std::vector<unsigned char> blk = slurp(argv[1]), raw = slurp(argv[2]);
        if (blk.empty() || raw.empty() || raw.size() % 24) { std::printf("input files\n"); return 3; }
        const size_t n = raw.size() / 24;
        std::vector<double> xyz(3 * n);
        std::memcpy(xyz.data(), raw.data(), raw.size());
        SDF::Octree oct;
        MemoryBlock mb;
        mb.size = blk.size(), mb.ptr = blk.data();
        oct.FromMemoryBlock(mb);
        std::vector<double> f(n), g(3 * n);
        oct.QueryGradient(xyz.data(), n, f.data(), g.data());
        for (size_t i = 0; i < n; ++i) std::printf("B %zu %016llx %016llx %016llx %016llx\n", i, bitsOf(f[i]), bitsOf(g[3 * i]), bitsOf(g[3 * i + 1]), bitsOf(g[3 * i + 2]));
        oct.QueryGradient(xyz.data(), n, f.data(), g.data(), true);
        for (size_t i = 0; i < n; ++i) std::printf("U %zu %016llx %016llx %016llx %016llx\n", i, bitsOf(f[i]), bitsOf(g[3 * i]), bitsOf(g[3 * i + 1]), bitsOf(g[3 * i + 2]));
        for (size_t i = 0; i < n && i < 40; ++i) {
            Eigen::Vector3d grad(7.0, 7.0, 7.0);
            const double v = oct.QueryGradient(Eigen::Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]), grad, i % 2 == 1);
            std::printf("S %zu %016llx %016llx %016llx %016llx\n", i, bitsOf(v), bitsOf(grad(0)), bitsOf(grad(1)), bitsOf(grad(2)));
        }
        const SDF::SurfaceMesh m = oct.ExtractSurface(oct.GetRootAABB(), Eigen::Vector3i(24, 24, 24));
        const std::vector<double> nrm = oct.SurfaceNormals(m);
        if (nrm.size() != m.vertices.size()) { std::printf("normal count\n"); return 4; }
        std::printf("M %zu %zu\n", m.vertices.size() / 3, m.triangles.size() / 3);
        for (size_t i = 0; i + 2 < nrm.size(); i += 3) {
            std::printf("V %zu %016llx %016llx %016llx\n", i / 3, bitsOf(m.vertices[i]), bitsOf(m.vertices[i + 1]), bitsOf(m.vertices[i + 2]));
            std::printf("N %zu %016llx %016llx %016llx\n", i / 3, bitsOf(nrm[i]), bitsOf(nrm[i + 1]), bitsOf(nrm[i + 2]));
        }
        if (!oct.SurfaceNormals(SDF::SurfaceMesh()).empty()) { std::printf("empty mesh\n"); return 5; }
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
