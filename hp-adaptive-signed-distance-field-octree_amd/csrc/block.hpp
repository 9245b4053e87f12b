// The serialised tree (Octree::ToMemoryBlock, Octree.cpp:424-456):
//   [u64 nCoeffs][f64 x nCoeffs][u64 nNodes][Node x nNodes][Config]
// Its layout, the reader every entry point that takes such bytes starts with, and the query mirror made from it.  Host only, header
// only; errors come back as a status and a message (the caller hands them to fail()).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "block_check.hpp"
#include "device_types.hpp"
#include "tables.hpp"

namespace hpsdf {

// ---- layout: byte offsets inside a block, and its size
constexpr size_t kBlockCoeffsAt = 8;
inline size_t blockNodeCountAt(uint64_t nCoeffs) { return kBlockCoeffsAt + 8 * (size_t)nCoeffs; }
inline size_t blockNodesAt(uint64_t nCoeffs) { return blockNodeCountAt(nCoeffs) + 8; }
inline size_t blockConfigAt(uint64_t nCoeffs, uint64_t nNodes) { return blockNodesAt(nCoeffs) + sizeof(hpsdf_node) * (size_t)nNodes; }
inline size_t blockBytes(uint64_t nCoeffs, uint64_t nNodes) {
    return 8 + 8 * (size_t)nCoeffs + 8 + sizeof(hpsdf_node) * (size_t)nNodes + sizeof(hpsdf_config);
}

// ---- a block whose counts agree with its size.  Not all of it is a view: the coefficients are read where they lie, the node array
// and the Config are copied out with memcpy, as every reader did before -- whoever indexes `nodes` needs no word on how the caller's
// bytes are aligned, and the copy stays valid while the continuity pass writes into the block
struct BlockView {
    uint64_t nCoeffs = 0, nNodes = 0;
    const double* coeffs = nullptr;  // inside the caller's block
    std::vector<hpsdf_node> nodes;   // a copy
    hpsdf_config cfg{};
};

// Untrusted bytes: no count is used as an offset before it has been compared with `size`, and no product of a count can wrap.
inline int readBlock(const void* block, size_t size, BlockView& v, std::string& err) {
    constexpr size_t kFixed = 16 + sizeof(hpsdf_config);  // the two counts and the Config
    if (!block || size < kFixed) {
        err = "block too small";
        return HPSDF_ERR_BAD_BLOCK;
    }
    const uint8_t* p = (const uint8_t*)block;
    std::memcpy(&v.nCoeffs, p, 8);
    if (v.nCoeffs > (size - kFixed) / 8) {
        err = "coefficient count exceeds block";
        return HPSDF_ERR_BAD_BLOCK;
    }
    std::memcpy(&v.nNodes, p + blockNodeCountAt(v.nCoeffs), 8);
    const size_t nodeBytes = size - kFixed - 8 * (size_t)v.nCoeffs;
    if (v.nNodes == 0 || nodeBytes / sizeof(hpsdf_node) != v.nNodes || nodeBytes % sizeof(hpsdf_node) != 0) {
        err = "node count does not match block size";
        return HPSDF_ERR_BAD_BLOCK;
    }
    v.coeffs = (const double*)(p + kBlockCoeffsAt);
    v.nodes.resize(v.nNodes);
    std::memcpy(v.nodes.data(), p + blockNodesAt(v.nCoeffs), sizeof(hpsdf_node) * v.nNodes);
    std::memcpy(&v.cfg, p + blockConfigAt(v.nCoeffs, v.nNodes), sizeof v.cfg);
    return HPSDF_OK;
}

// ---- the query mirror: what the descent of Query and its kin reads, on the device (hpsdf_tree_upload) and on the host (the *_block
// entry points) -- 8-byte records (interior: a = first child, b = kInteriorTag; leaf: a = offset of its coefficients in `padded`,
// b = degree) and the coefficients in walk order with every leaf on 128-byte lines of its own (the wave-cooperative fetch of
// query_general_kernel moves whole lines; a degree-2 leaf is one line, a degree-3 leaf two)
struct BlockMirror {
    std::vector<NodeRec> recs;
    std::vector<double> padded;
    BlockTreeInfo walk;  // leaves, maxDegree, maxDepth, minLeafDepth, depthOf, order
    double rootCentre[3], rootInvSizes[3];
};

// The descent recomputes every box from the root's and never reads one: a block is mirrored only if it is the dyadic octree over
// [-0.5,0.5]^3 that the descent assumes (HPSDF_ERR_UNSUPPORTED otherwise; HPSDF_ERR_BAD_BLOCK for a tree that is not one).
inline int mirrorBlock(const BlockView& v, const Tables& T, BlockMirror& m, std::string& err) {
    const std::vector<hpsdf_node>& nodes = v.nodes;
    const auto no = [&err](int code, const char* why) {
        err = why;
        return code;
    };
    if (v.nNodes > 0xFFFFFFF0ull) return no(HPSDF_ERR_BAD_BLOCK, "more nodes than a 32-bit record can index");
    if (v.nCoeffs > 0xFFFFFFFFull) return no(HPSDF_ERR_UNSUPPORTED, "more than 2^32 coefficients");
    if (nodes[0].degree != kInteriorDegree || nodes[0].child_idx == ~0ull)
        return no(HPSDF_ERR_UNSUPPORTED, "root must be an interior node (Octree::CreateRoot always splits it)");
    for (int a = 0; a < 3; ++a)
        if (nodes[0].aabb_min[a] != -0.5f || nodes[0].aabb_max[a] != 0.5f)
            return no(HPSDF_ERR_UNSUPPORTED, "internal root box must be [-0.5,0.5]^3 (Octree.cpp:798)");
    if (v.nNodes < 9) return no(HPSDF_ERR_BAD_BLOCK, "an interior root needs its 8 children");
    if (const int rc = checkBlockTree(nodes.data(), v.nNodes, v.nCoeffs, T.coeffCount, false, false, &m.walk, err)) return rc;
    m.recs.assign(v.nNodes, NodeRec{0, 0});
    m.padded.clear();
    m.padded.reserve(v.nCoeffs + 16 * v.nNodes);
    for (const uint64_t i : m.walk.order) {
        const hpsdf_node& n = nodes[i];
        if (n.degree == kInteriorDegree) {
            m.recs[i] = NodeRec{(uint32_t)n.child_idx, kInteriorTag};
            for (unsigned c = 0; c < 8; ++c) {
                const hpsdf_node& ch = nodes[n.child_idx + c];
                for (int d = 0; d < 3; ++d) {
                    const float mid = (n.aabb_max[d] + n.aabb_min[d]) * 0.5f;
                    const float emin = (c >> d) & 1u ? mid : n.aabb_min[d], emax = (c >> d) & 1u ? n.aabb_max[d] : mid;
                    if (ch.aabb_min[d] != emin || ch.aabb_max[d] != emax)
                        return no(HPSDF_ERR_UNSUPPORTED, "child boxes are not midpoint octants of their parent");
                }
            }
        } else {
            m.recs[i] = NodeRec{(uint32_t)m.padded.size(), (uint32_t)n.degree};
            m.padded.insert(m.padded.end(), v.coeffs + n.coeffs_start, v.coeffs + n.coeffs_start + T.coeffCount[n.degree]);
            m.padded.resize((m.padded.size() + 15) & ~(size_t)15, 0.0);
        }
    }
    if (m.padded.size() > 0xFFFFFFF0ull) return no(HPSDF_ERR_UNSUPPORTED, "more than 2^32 coefficients");
    for (int a = 0; a < 3; ++a) {
        m.rootCentre[a] = (double)((v.cfg.root_min[a] + v.cfg.root_max[a]) / 2.0f);    // Octree.cpp:419
        m.rootInvSizes[a] = (double)(1.0f / (v.cfg.root_max[a] - v.cfg.root_min[a]));  // Octree.cpp:420
    }
    return HPSDF_OK;
}

}  // namespace hpsdf
