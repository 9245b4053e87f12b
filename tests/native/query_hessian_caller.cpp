// A C++ caller of the drop-in's QueryHessian (scalar and batched) and SurfaceCurvature (tests/test_gpu_query_hessian.py compiles it with
// g++ the way tests/test_gpu_query_gradient.py compiles its caller): loads a MemoryBlock (argv[1]) and points (argv[2]: n x 3 doubles),
// prints every result as the 16 hex digits of its bits, one row a line:
//   "B i f gx gy gz hxx hyy hzz hxy hxz hyz mean gauss"   batched QueryHessian with curvature, unit off
//   "U i f gx gy gz hxx hyy hzz hxy hxz hyz"              batched, unit_ = true, curv = nullptr
//   "S i f gx gy gz hxx hyy hzz hxy hxz hyz mean gauss"   the scalar overload on the first 40 points (unit_ on odd rows)
//   "K i mean gauss"   SurfaceCurvature of ExtractSurface(root box, 24^3); "V i x y z" its vertices; "M nVerts nTris"
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

static void row(const char* tag, size_t i, const double* v, size_t count) {
    std::printf("%s %zu", tag, i);
    for (size_t k = 0; k < count; ++k) std::printf(" %016llx", bitsOf(v[k]));
    std::printf("\n");
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
        std::vector<double> f(n), g(3 * n), h(6 * n), k(2 * n);
        oct.QueryHessian(xyz.data(), n, f.data(), g.data(), h.data(), k.data());
        for (size_t i = 0; i < n; ++i) {
            double v[12] = {f[i], g[3 * i], g[3 * i + 1], g[3 * i + 2]};
            for (int e = 0; e < 6; ++e) v[4 + e] = h[6 * i + e];
            v[10] = k[2 * i], v[11] = k[2 * i + 1];
            row("B", i, v, 12);
        }
        oct.QueryHessian(xyz.data(), n, f.data(), g.data(), h.data(), nullptr, true);
        for (size_t i = 0; i < n; ++i) {
            double v[10] = {f[i], g[3 * i], g[3 * i + 1], g[3 * i + 2]};
            for (int e = 0; e < 6; ++e) v[4 + e] = h[6 * i + e];
            row("U", i, v, 10);
        }
        for (size_t i = 0; i < n && i < 40; ++i) {
            Eigen::Vector3d grad(7.0, 7.0, 7.0);
            double hess[6] = {7.0, 7.0, 7.0, 7.0, 7.0, 7.0};
            double mean = 7.0, gauss = 7.0;
            const double val = oct.QueryHessian(Eigen::Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]), grad, hess, i % 2 == 1, &mean, &gauss);
            double v[12] = {val, grad(0), grad(1), grad(2)};
            for (int e = 0; e < 6; ++e) v[4 + e] = hess[e];
            v[10] = mean, v[11] = gauss;
            row("S", i, v, 12);
        }
        const SDF::SurfaceMesh m = oct.ExtractSurface(oct.GetRootAABB(), Eigen::Vector3i(24, 24, 24));
        const std::vector<double> curv = oct.SurfaceCurvature(m);
        if (curv.size() * 3 != m.vertices.size() * 2) { std::printf("curvature count\n"); return 4; }
        std::printf("M %zu %zu\n", m.vertices.size() / 3, m.triangles.size() / 3);
        for (size_t i = 0; 3 * i + 2 < m.vertices.size(); ++i) {
            row("V", i, &m.vertices[3 * i], 3);
            row("K", i, &curv[2 * i], 2);
        }
        if (!oct.SurfaceCurvature(SDF::SurfaceMesh()).empty()) { std::printf("empty mesh\n"); return 5; }
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
