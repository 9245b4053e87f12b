// A C++ caller of the drop-in's ProjectToSurface (scalar and batched) and ProjectSurface (tests/test_gpu_project.py compiles it with g++
// the way tests/test_cxx_dropin.py compiles its callers): loads a MemoryBlock (argv[1]) and points (argv[2]: n x 3 doubles), prints every
// double as the 16 hex digits of its bits, one row a line:
//   "B i status iters x y z f gx gy gz"   batched ProjectToSurface (iso 0, tol 1e-9, 16 steps), world gradient
//   "U i status iters x y z f gx gy gz"   the same with unit_ = true, in place (outXyz = xyz)
//   "S i status iters x y z f gx gy gz"   the scalar overload on the first 40 points (odd i: unit_ = true)
//   "M nVerts nTris nMoved"               ExtractSurface(root box, 24^3) then ProjectSurface;  "V i x y z" its vertices afterwards
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

static void row(char tag, size_t i, int status, unsigned iters, const double* x, double f, const double* g) {
    std::printf("%c %zu %d %u %016llx %016llx %016llx %016llx %016llx %016llx %016llx\n", tag, i, status, iters, bitsOf(x[0]), bitsOf(x[1]),
                bitsOf(x[2]), bitsOf(f), bitsOf(g[0]), bitsOf(g[1]), bitsOf(g[2]));
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
        std::vector<double> x(3 * n), f(n), g(3 * n);
        std::vector<uint8_t> it(n), st(n);
        oct.ProjectToSurface(xyz.data(), n, x.data(), 0.0, 1e-9, 16, f.data(), g.data(), it.data(), st.data());
        for (size_t i = 0; i < n; ++i) row('B', i, st[i], it[i], &x[3 * i], f[i], &g[3 * i]);
        x = xyz;
        oct.ProjectToSurface(x.data(), n, x.data(), 0.0, 1e-9, 16, f.data(), g.data(), it.data(), st.data(), true);
        for (size_t i = 0; i < n; ++i) row('U', i, st[i], it[i], &x[3 * i], f[i], &g[3 * i]);
        for (size_t i = 0; i < n && i < 40; ++i) {
            Eigen::Vector3d p(7.0, 7.0, 7.0), grad(7.0, 7.0, 7.0);
            double v = 7.0;
            uint32_t k = 7;
            const int s = oct.ProjectToSurface(Eigen::Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]), p, 0.0, 1e-9, 16, &v, &grad, i % 2 == 1, &k);
            const double px[3] = {p(0), p(1), p(2)}, pg[3] = {grad(0), grad(1), grad(2)};
            row('S', i, s, k, px, v, pg);
        }
        Eigen::Vector3d only;
        if (oct.ProjectToSurface(Eigen::Vector3d(0.1, -0.2, 0.3), only) > HPSDF_PROJECT_FLAT) { std::printf("defaults\n"); return 4; }
        SDF::SurfaceMesh m = oct.ExtractSurface(oct.GetRootAABB(), Eigen::Vector3i(24, 24, 24));
        const std::vector<u64> tris = m.triangles;
        const unsigned long long moved = oct.ProjectSurface(m, oct.GetRootAABB(), Eigen::Vector3i(24, 24, 24));
        if (tris != m.triangles) { std::printf("triangles changed\n"); return 5; }
        std::printf("M %zu %zu %llu\n", m.vertices.size() / 3, m.triangles.size() / 3, moved);
        for (size_t i = 0; i + 2 < m.vertices.size(); i += 3)
            std::printf("V %zu %016llx %016llx %016llx\n", i / 3, bitsOf(m.vertices[i]), bitsOf(m.vertices[i + 1]), bitsOf(m.vertices[i + 2]));
        SDF::SurfaceMesh none;
        if (oct.ProjectSurface(none, oct.GetRootAABB(), Eigen::Vector3i(24, 24, 24)) != 0) { std::printf("empty mesh\n"); return 6; }
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
