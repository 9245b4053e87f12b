// A C++ caller of the drop-in's CastRay and CastRays (tests/test_gpu_cast_rays.py compiles it with g++ the way tests/test_cxx_dropin.py
// compiles its callers): loads a MemoryBlock (argv[1]) and rays (argv[2]: n x 7 doubles -- origin, direction, t_max), prints every
// double as the 16 hex digits of its bits, one row a line:
//   "B i status evals cells t x y z f gx gy gz"   batched CastRays (iso 0, tol 1e-9, the defaults), world gradient
//   "U i status evals cells t x y z f gx gy gz"   the same with unit_ = true
//   "S i status 0 0 t x y z f gx gy gz"           the scalar CastRay on the first 40 rays (odd i: unit_ = true)
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

static void row(char tag, size_t i, int status, unsigned evals, unsigned cells, double t, const double* x, double f, const double* g) {
    std::printf("%c %zu %d %u %u %016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx\n", tag, i, status, evals, cells, bitsOf(t),
                bitsOf(x[0]), bitsOf(x[1]), bitsOf(x[2]), bitsOf(f), bitsOf(g[0]), bitsOf(g[1]), bitsOf(g[2]));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        std::vector<unsigned char> blk = slurp(argv[1]), raw = slurp(argv[2]);
        if (blk.empty() || raw.empty() || raw.size() % 56) { std::printf("input files\n"); return 3; }
        const size_t n = raw.size() / 56;
        std::vector<double> o(3 * n), d(3 * n), tm(n);
        for (size_t i = 0; i < n; ++i) {
            std::memcpy(&o[3 * i], raw.data() + 56 * i, 24);
            std::memcpy(&d[3 * i], raw.data() + 56 * i + 24, 24);
            std::memcpy(&tm[i], raw.data() + 56 * i + 48, 8);
        }
        SDF::Octree oct;
        MemoryBlock mb;
        mb.size = blk.size(), mb.ptr = blk.data();
        oct.FromMemoryBlock(mb);
        std::vector<double> t(n), x(3 * n), f(n), g(3 * n);
        std::vector<uint8_t> st(n);
        std::vector<uint16_t> ev(n), ce(n);
        oct.CastRays(o.data(), d.data(), tm.data(), n, st.data(), t.data(), x.data(), f.data(), g.data(), ev.data(), ce.data());
        for (size_t i = 0; i < n; ++i) row('B', i, st[i], ev[i], ce[i], t[i], &x[3 * i], f[i], &g[3 * i]);
        oct.CastRays(o.data(), d.data(), tm.data(), n, st.data(), t.data(), x.data(), f.data(), g.data(), ev.data(), ce.data(), 0.0, 1e-9, 32,
                     4096, true);
        for (size_t i = 0; i < n; ++i) row('U', i, st[i], ev[i], ce[i], t[i], &x[3 * i], f[i], &g[3 * i]);
        for (size_t i = 0; i < n && i < 40; ++i) {
            Eigen::Vector3d p(7.0, 7.0, 7.0), grad(7.0, 7.0, 7.0);
            double v = 7.0, ti = 7.0;
            const SDF::Ray ray(Eigen::Vector3d(o[3 * i], o[3 * i + 1], o[3 * i + 2]), Eigen::Vector3d(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
            const int s = oct.CastRay(ray, tm[i], ti, &p, &grad, 0.0, 1e-9, 32, 4096, i % 2 == 1, &v);
            const double px[3] = {p(0), p(1), p(2)}, pg[3] = {grad(0), grad(1), grad(2)};
            row('S', i, s, 0, 0, ti, px, v, pg);
        }
        double only = 0.0;
        const SDF::Ray axis(Eigen::Vector3d(-2.0, 0.01, 0.02), Eigen::Vector3d(1.0, 0.0, 0.0));
        if (oct.CastRay(axis, 10.0, only) > HPSDF_CAST_INVALID) { std::printf("defaults\n"); return 4; }
        oct.CastRays(nullptr, nullptr, nullptr, 0, nullptr);
        return 0;
    } catch (const SDF::Error& e) {
        std::printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
