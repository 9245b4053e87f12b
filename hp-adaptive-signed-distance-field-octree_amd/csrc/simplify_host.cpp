// Simplify on the calling thread (include/hpsdf.h, "Simplify"): the levels and the candidates of simplify.hip's driver, walked serially
// with simplify.hpp's statements -- the same bytes, no device.  Also the argument check both paths share and the table getter.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "block.hpp"
#include "runtime.hpp"
#include "simplify.hpp"

namespace hpsdf {

int simplifyArgumentError(double rms, uint32_t flags, const void* outBlock, const void* outSize) {
    if (!outBlock || !outSize) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_simplify: null output");
    if (!(rms >= 0.0) || !(rms <= DBL_MAX)) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_simplify: rms must be finite and >= 0");
    if (flags & ~kSimpFlags) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_simplify: unknown flag bits");
    return HPSDF_OK;
}

namespace {

struct HostMerge {
    const Tables& T;
    const BlockView& v;
    SimpState& s;
    uint8_t bidx[kMaxCoeffs][3];
    std::vector<double> U, V;
    double P[kMaxCoeffs], acc[512];

    HostMerge(const Tables& t, const BlockView& view, SimpState& st) : T(t), v(view), s(st), U(kSimpQ * kSimpQ * kSimpQ), V(kSimpQ * kSimpQ * kSimpQ) {
        for (int e = 0; e < kMaxCoeffs; ++e)
            for (int k = 0; k < 3; ++k) bidx[e][k] = (uint8_t)T.basisIndex[e][k];
    }
    const double* rowsOf(const SimpNode& n) const { return n.rowsAt < v.nCoeffs ? v.coeffs + n.rowsAt : s.ext.data() + (n.rowsAt - v.nCoeffs); }

    // One candidate: the kernel's phases with e running serially where the kernel has lanes.  true: merged.
    bool candidate(uint32_t node, double rms) {
        using C = SimpCube<kSimpQ>;
        const double* Tr = &T.transfer[0][0][0];
        SimpNode& parent = s.nodes[node];
        const SimpNode* ch = &s.nodes[parent.child];
        uint32_t q = 0;
        for (int n = 0; n < 8; ++n) {
            if (ch[n].degree == kInteriorDegree) return false;
            q = q > ch[n].degree ? q : ch[n].degree;
        }
        const uint32_t entries = simpEntries(q), stored = (uint32_t)T.coeffCount[q], p2 = simpPow2(entries);
        for (uint32_t e = 0; e < entries; ++e) P[e] = 0.0;
        for (uint32_t n = 0; n < 8u; ++n) {
            const double* c = rowsOf(ch[n]);
            const uint32_t have = (uint32_t)T.coeffCount[ch[n].degree];
            for (uint32_t e = 0; e < entries; ++e) U[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = e < have ? c[e] : 0.0;
            for (uint32_t e = 0; e < entries; ++e) V[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = C::fwdX(Tr, n, U.data(), bidx[e][0], bidx[e][1], bidx[e][2]);
            for (uint32_t e = 0; e < entries; ++e) U[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = C::fwdY(Tr, n, V.data(), bidx[e][0], bidx[e][1], bidx[e][2]);
            for (uint32_t e = 0; e < entries; ++e) P[e] = P[e] + C::fwdZ(Tr, n, U.data(), bidx[e][0], bidx[e][1], bidx[e][2]);
        }
        for (uint32_t e = stored; e < entries; ++e) P[e] = 0.0;  // (degree 6 stores 83 of its 84 entries)
        for (uint32_t t = 0; t < p2; ++t) acc[t] = 0.0;
        double carried = 0.0;
        for (uint32_t n = 0; n < 8u; ++n) {
            const double* c = rowsOf(ch[n]);
            const uint32_t have = (uint32_t)T.coeffCount[ch[n].degree];
            for (uint32_t e = 0; e < entries; ++e) U[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = P[e];
            for (uint32_t e = 0; e < entries; ++e) V[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = C::bwdZ(Tr, n, U.data(), (int)q, bidx[e][0], bidx[e][1], bidx[e][2]);
            for (uint32_t e = 0; e < entries; ++e) U[C::at(bidx[e][0], bidx[e][1], bidx[e][2])] = C::bwdY(Tr, n, V.data(), (int)q, bidx[e][0], bidx[e][1], bidx[e][2]);
            for (uint32_t e = 0; e < entries; ++e) {
                const double d = (e < have ? c[e] : 0.0) - C::bwdX(Tr, n, U.data(), (int)q, bidx[e][0], bidx[e][1], bidx[e][2]);
                acc[e] = acc[e] + d * d;
            }
            carried = carried + ch[n].e;
        }
        const double b = simpBound(simpReduce(acc, p2), carried);
        if (!simpAccept(b, rms, parent.depth)) return false;
        parent.rowsAt = v.nCoeffs + s.ext.size();
        parent.degree = (uint8_t)q;
        parent.e = b;
        s.ext.insert(s.ext.end(), P, P + stored);
        return true;
    }
};

}  // namespace

// The passes over a state simplifyBegin made.
void simplifyOnHost(const BlockView& v, const BlockMirror& m, const Tables& T, double rms, uint32_t flags, SimpState& s) {
    if (rms == 0.0) return;
    if (flags & HPSDF_SIMPLIFY_MERGE) {
        HostMerge hm(T, v, s);
        s.ext.reserve(s.extBound);  // (rowsOf's pointers stay valid while a level appends)
        for (int D = m.walk.maxDepth; D >= 2; --D) {
            bool any = false;
            for (const uint32_t node : s.level[D - 1]) {
                const SimpNode* ch = &s.nodes[s.nodes[node].child];
                bool cand = true;
                for (int n = 0; n < 8; ++n) cand = cand && ch[n].degree != kInteriorDegree;
                if (!cand) continue;
                any = true;
                hm.candidate(node, rms);
            }
            s.levels += any ? 1 : 0;
        }
    }
    if (flags & HPSDF_SIMPLIFY_TRUNCATE) {
        std::vector<uint32_t> leaves;
        simplifyLeaves(s, leaves);
        for (const uint32_t i : leaves) {
            SimpNode& n = s.nodes[i];
            const double* c = n.rowsAt < v.nCoeffs ? v.coeffs + n.rowsAt : s.ext.data() + (n.rowsAt - v.nCoeffs);
            const uint32_t d = simpTruncate(c, n.degree, T.coeffCount, rms, n.depth, &n.e);
            s.truncations += d != n.degree ? 1 : 0;
            n.degree = (uint8_t)d;
        }
    }
}

}  // namespace hpsdf

using namespace hpsdf;

extern "C" int hpsdf_simplify_block(const void* block, size_t size, double rms, uint32_t flags, void** out_block, size_t* out_size,
                                    hpsdf_simplify_stats* stats) {
    HPSDF_TRY
    if (const int rc = simplifyArgumentError(rms, flags, out_block, out_size)) return rc;
    const Tables& T = tables();
    BlockView v;
    BlockMirror m;
    std::string why;
    int rc = readBlock(block, size, v, why);
    if (!rc) rc = mirrorBlock(v, T, m, why);
    if (rc) return fail(rc, why);
    SimpState s;
    simplifyBegin(v, m, T, s);
    simplifyOnHost(v, m, T, rms, flags, s);
    rc = simplifyAssemble(v, T, s, [](size_t n) { return std::malloc(n); }, out_block, out_size, stats, why);
    return rc ? fail(rc, why) : HPSDF_OK;
    HPSDF_CATCH
}

extern "C" int hpsdf_simplify_transfer(double out[2][13][13]) {
    if (!out) return fail(HPSDF_ERR_INVALID_ARGUMENT, "hpsdf_simplify_transfer: null output");
    std::memcpy(out, tables().transfer, sizeof tables().transfer);
    return HPSDF_OK;
}
