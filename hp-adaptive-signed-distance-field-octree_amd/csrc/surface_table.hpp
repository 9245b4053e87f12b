// Case table of hpsdf_extract_surface (include/hpsdf.h), generated at compile time by a face-local rule: one source for the
// host copy (hpsdf_surface_case_table) and the device's packed copy (surface.hip).
//
// Corners c = dx + 2 dy + 4 dz.  Cube-local edges: x 0->1, 2->3, 4->5, 6->7 (0..3); y 0->2, 1->3, 4->6, 5->7 (4..7);
// z 0->4, 1->5, 2->6, 3->7 (8..11).  On every face, walked counter-clockwise as seen from outside the cube, an edge whose walk
// enters an inside corner is joined by a segment to the next crossing edge of the walk (which leaves one): one segment around an
// odd corner, one across two adjacent inside corners, and two for diagonal inside corners -- each cutting one inside corner off.
// Every crossing edge lies on two faces and starts a segment on exactly one of them, so the segments close into loops; each loop,
// listed from its smallest edge, is fan-triangulated from its first edge whose diagonals all leave the cube's faces (a chord in a
// face could be drawn by the neighbouring cube too).  A triangle then winds counter-clockwise seen from the side where values are
// >= iso.
#pragma once
#include <cstdint>

namespace hpsdf {

constexpr int kSurfaceMaxTris = 5;  // the rule's largest case
constexpr int kSurfaceRow = 16;     // 5 x 3 edges and a -1 terminator

struct SurfaceTable {
    int8_t rows[256][kSurfaceRow];
    uint8_t count[256];
    // device form: bits 0-2 the triangle count, then 4 bits a cube-local edge, triangle t's edge m at bit 3 + 12 t + 4 m
    uint64_t packed[256];
    bool faceFreeFans;  // every loop found an apex whose diagonals leave the faces
};

constexpr int surfaceEdgeOf(int a, int b) {  // cube-local edge between corners a < b (adjacent), or -1
    const int d = a ^ b;
    if (d == 1) return (a >> 1) & 3;                          // x: pair (a, a + 1) -> edge a / 2
    if (d == 2) return 4 + ((a & 1) | ((a >> 2) & 1) << 1);   // y: 0->2, 1->3, 4->6, 5->7
    if (d == 4) return 8 + (a & 3);                           // z: 0->4 .. 3->7
    return -1;
}

constexpr bool surfaceShareFace(int e0, int e1) {  // two cube-local edges on one face of the cube
    const int c0[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
    const int a0 = e0 >> 2, a1 = e1 >> 2;
    const int p0 = c0[e0], q0 = p0 | (1 << a0), p1 = c0[e1], q1 = p1 | (1 << a1);
    for (int a = 0; a < 3; ++a)
        for (int s = 0; s < 2; ++s)
            if (((p0 >> a) & 1) == s && ((q0 >> a) & 1) == s && ((p1 >> a) & 1) == s && ((q1 >> a) & 1) == s) return true;
    return false;
}

constexpr SurfaceTable makeSurfaceTable() {
    SurfaceTable T{};
    T.faceFreeFans = true;
    for (int cs = 0; cs < 256; ++cs) {
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        for (int a = 0; a < 3; ++a) {
            for (int side = 0; side < 2; ++side) {
                const int u = (a + 1) % 3, v = (a + 2) % 3;
                // counter-clockwise seen from outside: (u, v, +a) is right-handed, so side 1 walks (0,0) (1,0) (1,1) (0,1) in (u, v);
                // side 0 looks from -a and walks the other way round
                const int wu1[4] = {0, 1, 1, 0}, wv1[4] = {0, 0, 1, 1};
                int q[4] = {0, 0, 0, 0};
                for (int k = 0; k < 4; ++k) {
                    const int du = side ? wu1[k] : wv1[k], dv = side ? wv1[k] : wu1[k];
                    q[k] = (side << a) | (du << u) | (dv << v);
                }
                for (int k = 0; k < 4; ++k) {
                    const int c0 = q[k], c1 = q[(k + 1) & 3];
                    const bool in0 = (cs >> c0) & 1, in1 = (cs >> c1) & 1;
                    if (in0 || !in1) continue;  // not an entering edge
                    for (int s = 1; s < 4; ++s) {
                        const int d0 = q[(k + s) & 3], d1 = q[(k + s + 1) & 3];
                        if ((((cs >> d0) & 1) != 0) != (((cs >> d1) & 1) != 0)) {
                            const int e0 = surfaceEdgeOf(c0 < c1 ? c0 : c1, c0 < c1 ? c1 : c0);
                            const int e1 = surfaceEdgeOf(d0 < d1 ? d0 : d1, d0 < d1 ? d1 : d0);
                            next[e0] = e1;
                            break;
                        }
                    }
                }
            }
        }
        bool seen[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
        int n = 0;
        for (int e = 0; e < 12; ++e) {
            if (next[e] < 0 || seen[e]) continue;
            int loop[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int len = 0;
            for (int f = e; !seen[f]; f = next[f]) {
                seen[f] = true;
                loop[len++] = f;
            }
            // the fan's apex: the first loop edge (in loop order from the smallest) none of whose diagonals joins two edges of one
            // cube face -- such a chord would lie in the face, where the neighbouring cube can draw it too (an edge of four triangles)
            int apex = -1;
            for (int s0 = 0; s0 < len; ++s0) {
                bool clean = true;
                for (int i = 2; i + 1 < len && clean; ++i) clean = !surfaceShareFace(loop[s0], loop[(s0 + i) % len]);
                if (clean) {
                    apex = s0;
                    break;
                }
            }
            if (apex < 0) T.faceFreeFans = false, apex = 0;
            for (int i = 1; i + 1 < len; ++i) {
                T.rows[cs][3 * n] = (int8_t)loop[apex];
                T.rows[cs][3 * n + 1] = (int8_t)loop[(apex + i) % len];
                T.rows[cs][3 * n + 2] = (int8_t)loop[(apex + i + 1) % len];
                ++n;
            }
        }
        for (int i = 3 * n; i < kSurfaceRow; ++i) T.rows[cs][i] = -1;
        T.count[cs] = (uint8_t)n;
        uint64_t p = (uint64_t)n;
        for (int i = 0; i < 3 * n; ++i) p |= (uint64_t)T.rows[cs][i] << (3 + 4 * i);
        T.packed[cs] = p;
    }
    return T;
}

}  // namespace hpsdf
