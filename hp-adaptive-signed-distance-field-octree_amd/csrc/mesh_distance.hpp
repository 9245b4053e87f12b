// The f32 signed distance to a triangle mesh: closest point on a triangle, pseudo-normals, and the traversals of the BVH (per point,
// per wave, per wave with a shared pool).  Device code that also compiles for the host.  Included by mesh_field.hip (the mesh
// kernels and the host path) and, through field_glue.hpp, by the fit units (fit_mesh.hip is the one that instantiates it).
// The functions that are not forced inline are `static`: a header's functions need internal linkage, and the device
// compiler internalises every function of a code object anyway, so each unit's copy compiles as it did in one file.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "acosf_host_libm.hpp"
#include "device_types.hpp"

namespace hpsdf {

// ---- mesh signed distance (all f32) ----------------------------------------
// Source/Meshing/Utility.cpp:5-97, Source/Meshing/Mesh.cpp:54-63,162-242.
// The per-point path below (closest-point routine, pseudo-normals, bounds, the stack traversal) also compiles for the HOST: calls of a
// few points on a plain mesh field are answered on the calling thread from a host copy of the field's arrays (meshEvalHostPoints,
// mesh_field.hip) -- same statements, -ffp-contract=off on both sides, IEEE divide and square root: the device's bits.
#define HPSDF_HD __host__ __device__
// a bound's square root: the raw 1-ulp instruction on the device, sqrtf on the host (bounds only have to be conservative; their slack is
// four orders of magnitude wider than either)
HPSDF_HD __forceinline__ float boundSqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}
struct V3 {
    float x, y, z;
};
HPSDF_HD __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
HPSDF_HD __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
HPSDF_HD __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
HPSDF_HD __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
HPSDF_HD __forceinline__ V3 cross(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
HPSDF_HD __forceinline__ float sqnorm(V3 a) { return a.x * a.x + (a.y * a.y + a.z * a.z); }
HPSDF_HD __forceinline__ V3 normalized(V3 a) {
    const float z = sqnorm(a);
    if (z > 0.0f) {
        const float n = sqrtf(z);
        return {a.x / n, a.y / n, a.z / n};
    }
    return a;
}
HPSDF_HD __forceinline__ V3 meshVert(const MeshDev& m, uint32_t i) {
    return {m.verts[3 * i], m.verts[3 * i + 1], m.verts[3 * i + 2]};
}

constexpr float kEpsF32 = 0.000001f;  // Include/Utility/Literals.h:13

// A query point with a coordinate that is not a finite number has no closest triangle: every comparison of the reference's
// search fails, its bestTri stays -1 and Mesh::SignedDistanceAtPt reads out of bounds (Mesh.cpp:139,157; BVH.cpp:281,343).
// Here such a point takes no part in a traversal and its value is this NaN, on every path.
HPSDF_HD __forceinline__ bool meshPointFinite(V3 p) { return fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX && fabsf(p.z) <= FLT_MAX; }
HPSDF_HD __forceinline__ float meshNoTriangle() { return hpsdfAcosfBits(0xFFFFFFFFu); }

// What closestSimplex falls back on when the reference's face case has left the triangle: the point the weights describe lies outside,
// so the triangle's closest point is on its boundary -- the nearest of the closest points of its three edges (a + t ab, t the clamped
// projection: well conditioned in f32 whatever the triangle's shape; ties go to ab, then bc, then ca).  A function of its own, called:
// inlined into closestSimplex's five copies inside mesh_sample_kernel it made the kernel 14 % slower WITHOUT ever running (3 000 more
// instructions in the hot loops: the instruction cache), behind a call 3 % (2.1 M-triangle torus at 1e-6: 30.5 ms without any of
// this, 34.5 inlined, 31.6 called).  (If the weights were wrong -- cancellation on a needle, the point really inside -- the answer is off by
// at most the needle's width, upwards: a distance that is too large never breaks a bound.)
inline HPSDF_HD __noinline__ int closestOnBoundary(V3 pt, V3 a, V3 b, V3 c, V3& q) {
    int code = 0;
    float best = __builtin_inff();
    auto edge = [&](V3 p0, V3 p1, int edgeCode, int v0, int v1) {
        const V3 e = p1 - p0;
        const float den = dot(e, e);
        float t = den > 0.0f ? dot(pt - p0, e) / den : 0.0f;
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        const V3 x = p0 + t * e;
        const float d = sqnorm(pt - x);
        if (d < best) best = d, q = x, code = t <= 0.0f ? v0 : (t >= 1.0f ? v1 : edgeCode);
    };
    edge(a, b, 4, 0, 1);
    edge(b, c, 5, 1, 2);
    edge(a, c, 6, 0, 2);
    if (!(best < __builtin_inff())) q = a, code = 0;  // (nothing finite: the vertex, like the reference's first case)
    return code;
}

// returns simplex*4 + simplexIdx; closest point in q
// (n: the triangle's unnormalised normal cross(b - a, c - a), precomputed per triangle by mesh_tripos_kernel with these very
// operations -- the value the reference recomputes in every call, Utility.cpp:41)
// The reference's routine, operation by operation, with ONE stated exception (`tol`, a distance: a quarter of the traversal's
// slack).  Vertex and edge cases return points OF the triangle (a vertex; a + t ab with 0 < t < 1).  The face case forms
// q = u a + v b + w c from barycentric quotients and returns it whatever the weights are: the absolute 1e-6 guards of the edge tests
// (snom > eps ...) are lengths SQUARED, so beside a short edge of a needle they let points through that lie well outside the
// triangle -- q is then a point of the triangle's PLANE, up to eps / (shortest altitude) away from it, and its distance lies
// BELOW the triangle's.  No bound can be a bound on that: a search that comes across the needle returns the artefact, one that has
// pruned it (by its box, rightly) does not, and two traversals disagree (tools/fuzz_mesh_bvh.py seeds 100758, 501177: a sphere
// squashed 1000 : 1).  The weights say exactly where q is -- a negative weight m puts it |m| altitudes beyond the opposite edge,
// i.e. |m| |n| / |edge| outside -- so: a face-case point farther than `tol` outside its triangle is not taken by a search that could
// make it its best (`best`: the caller's squared distance so far); it takes the boundary's closest point instead (closestOnBoundary).  Every traversal and the O(n) scan kernel share this function, so they
// agree bit for bit on every mesh; against the reference the value differs exactly where the reference's is such an artefact.
inline HPSDF_HD int closestSimplex(V3 pt, V3 a, V3 b, V3 c, V3 n, float tol, float best, V3& q) {
    const V3 ab = b - a, ac = c - a, bc = c - b;
    const float snom = dot(pt - a, ab), sdenom = dot(pt - b, a - b);
    const float tnom = dot(pt - a, ac), tdenom = dot(pt - c, a - c);
    if (snom < kEpsF32 && tnom < kEpsF32) {
        q = a;
        return 0;
    }
    const float unom = dot(pt - b, bc), udenom = dot(pt - c, b - c);
    if (sdenom < kEpsF32 && unom < kEpsF32) {
        q = b;
        return 1;
    }
    if (tdenom < kEpsF32 && udenom < kEpsF32) {
        q = c;
        return 2;
    }
    const float vc = dot(n, cross(a - pt, b - pt));
    if (vc < kEpsF32 && snom > kEpsF32 && sdenom > kEpsF32) {
        q = a + (snom / (snom + sdenom)) * ab;
        return 4;
    }
    const float va = dot(n, cross(b - pt, c - pt));
    if (va < kEpsF32 && unom > kEpsF32 && udenom > kEpsF32) {
        q = b + (unom / (unom + udenom)) * bc;
        return 5;
    }
    const float vb = dot(n, cross(c - pt, a - pt));
    if (vb < kEpsF32 && tnom > kEpsF32 && tdenom > kEpsF32) {
        q = a + (tnom / (tnom + tdenom)) * ac;
        return 6;
    }
    const float u = va / (va + vb + vc);
    const float v = vb / (va + vb + vc);
    const float w = 1.0f - u - v;
    q = (u * a + v * b) + w * c;
    const float m = fminf(u, fminf(v, w));  // (NaN weights -- a triangle without area -- stay the reference's NaN point)
    // Two cheap tests in front, for every face-case result.  The weight alone: an altitude is at most the mesh's extent E and
    // tol = 5e-7 max(E, largest coordinate), so a weight above -5e-7 cannot put q more than tol outside.  And whether the value could
    // win at all (d <= best; ties count, they go to the lower triangle index): one that cannot is left as it is -- the triangle's
    // proper distance is larger still, so it loses either way.  On a fine mesh negative weights are the rule, not the exception (the
    // reference's absolute guards send most outside points of a small triangle here), but a test beats its caller's best once or twice
    // per search: what passes both is measured exactly, and the three divisions of closestOnBoundary are spent on potential winners
    // only.  (Substituting at the call sites instead of here cost 18 VGPRs and a wave per SIMD.)  best = +inf passes
    // everything: the winner's recomputation, which must equal what the search stored for it (a winner whose face-case point had left
    // the triangle was, by this rule, substituted when it won).
    if (m < -5e-7f && sqnorm(pt - q) <= best) {
        const float e2 = m == u ? sqnorm(bc) : (m == v ? sqnorm(ac) : sqnorm(ab));  // the edge opposite the negative weight
        if ((m * m) * sqnorm(n) > (tol * tol) * e2) return closestOnBoundary(pt, a, b, c, q);
    }
    return 8;
}

inline HPSDF_HD V3 faceNormal(const MeshDev& m, uint32_t t) {
    const V3 a = meshVert(m, m.tris[3 * t]), b = meshVert(m, m.tris[3 * t + 1]), c = meshVert(m, m.tris[3 * t + 2]);
    return normalized(cross(b - a, c - a));
}

inline HPSDF_HD V3 pseudoNormal(const MeshDev& m, uint32_t t, int code) {
    const int simplex = code >> 2, sidx = code & 3;
    if (simplex == 2) return faceNormal(m, t);
    if (simplex == 1) {  // Mesh.cpp:201-215
        const uint32_t adj = m.halfEdges[3 * t + sidx] / 3;
        const float pif = (float)3.14159265359;
        return normalized(pif * faceNormal(m, t) + pif * faceNormal(m, adj));
    }
    // vertex: walk the half-edge fan, Mesh.cpp:218-242
    V3 n = {0.0f, 0.0f, 0.0f};
    uint32_t he = 3 * t + sidx, cur = t;
    int guard = 0;
    do {
        const V3 t0 = meshVert(m, m.tris[3 * cur]), t1 = meshVert(m, m.tris[3 * cur + 1]), t2 = meshVert(m, m.tris[3 * cur + 2]);
        const int k = he % 3;  // (selected, not indexed: an indexed array of registers lives in scratch memory)
        const V3 pk = k == 0 ? t0 : (k == 1 ? t1 : t2), pk1 = k == 0 ? t1 : (k == 1 ? t2 : t0), pk2 = k == 0 ? t2 : (k == 1 ? t0 : t1);
        const V3 ab = pk1 - pk;
        const V3 ac = pk2 - pk;
        const float ang = hpsdfAcosf(dot(normalized(ab), normalized(ac)));  // std::acos of the HOST's libm, bit for bit
        n = n + ang * faceNormal(m, cur);
        he = m.halfEdges[he];
        he = ((he % 3) == 2) ? (he - 2) : (he + 1);
        cur = he / 3;
    } while (cur != t && ++guard < 4096);
    return normalized(n);
}

// A leaf reference (BvhNode::c0 / c1 < 0): its first slot and how many, and the triangle a slot holds.
HPSDF_HD __forceinline__ uint32_t leafFirst(int32_t c) { return (uint32_t)~c >> kMeshLeafShift; }
HPSDF_HD __forceinline__ uint32_t leafCount(int32_t c) { return ((uint32_t)~c & (kMeshLeafMax - 1u)) + 1u; }
// A triPre record (three float4 per leaf slot): g.xyz hu | n.xyz hv | u.xyz triangle -- the triangle lies in the plane through g
// across the unit normal n, inside the rectangle |u . (x - g)| <= hu, |v . (x - g)| <= hv of that plane (u a unit vector along its
// longest edge, v = n x u).  n = u = 0, hu = 0, hv = rho degrades it to the ball of radius rho around g (slivers whose normal cancels).
struct TriPre {
    float4 g, n, u;
};
HPSDF_HD __forceinline__ TriPre loadTriPre(const MeshDev& m, uint32_t slot) {
    return TriPre{m.triPre[3 * (size_t)slot], m.triPre[3 * (size_t)slot + 1], m.triPre[3 * (size_t)slot + 2]};
}
HPSDF_HD __forceinline__ uint32_t triPreTriangle(const TriPre& r) { return hpsdfAcosfWord(r.u.w); }
HPSDF_HD __forceinline__ uint32_t slotTriangle(const MeshDev& m, uint32_t slot) { return hpsdfAcosfWord(m.triPre[3 * (size_t)slot + 2].w); }

// The lower-bound test on a triPre record: with s = n . (p - g) and a = u . (p - g) the squared distance of p from the triangle is
// at least s^2 + max(|a| - hu, 0)^2 + max(sqrt(|p - g|^2 - s^2 - a^2) - hv, 0)^2 -- two dozen instructions against the two hundred
// of the closest-point test.  (Until the middle of round 3 the triangle was bounded by a circle in its plane; the rectangle costs
// five instructions more and has half the area for the 4 : 1 triangles of a stretched grid: 17 -> 10 candidates per sample on
// the displaced torus with the final distance known; no change on equilateral triangles.)
// A box only says "the triangle is somewhere in here": for a sample at distance D from a surface tessellated at size h every
// triangle whose box dips into the ball passes the box test, a patch ~sqrt(2 D h) wide (~300 triangles per sample on a
// 1.3 M-triangle sphere); the plane-and-rectangle bound leaves the ones within ~h.
// A triangle is dropped only if the bound exceeds the best distance by `slack` = 2e-6 of the mesh's scale (its extent, or
// its largest coordinate if that is larger: f32 positions round at that scale; meshSlack has the error budget) and by
// 5e-6 of itself -- so the winner is still exactly the exhaustive scan's (test_mesh_bvh_equals_linear_scan_bitwise, the
// fuzzers).  rejectBound = what the bound is compared with; a NaN bound never drops anything.
// (Bounds, unlike the closest-point arithmetic, need not follow the reference operation by operation: their dot products
// are fused multiply-adds -- three instructions instead of five -- and the square root is the raw v_sqrt_f32, 1 ulp; the
// slack they are compared with is four orders of magnitude wider than either.)
HPSDF_HD __forceinline__ float dotF(V3 a, V3 b) { return __builtin_fmaf(a.x, b.x, __builtin_fmaf(a.y, b.y, a.z * b.z)); }
HPSDF_HD __forceinline__ float triLowerBound2(V3 p, const TriPre& r) {
    const V3 dx = p - V3{r.g.x, r.g.y, r.g.z};
    const float sd = dotF(V3{r.n.x, r.n.y, r.n.z}, dx), ad = dotF(V3{r.u.x, r.u.y, r.u.z}, dx);
    const float lat2 = __builtin_fmaf(-ad, ad, __builtin_fmaf(-sd, sd, dotF(dx, dx)));
    const float ou = fmaxf(fabsf(ad) - r.g.w, 0.0f);
    const float ov = fmaxf(boundSqrt(fmaxf(lat2, 0.0f)) - r.n.w, 0.0f);
    return __builtin_fmaf(ov, ov, __builtin_fmaf(ou, ou, sd * sd));
}
// The slack (a distance) a lower bound must exceed the best distance by before anything is dropped.  What it has to cover
// (u = 2^-24, D the distance, M the largest coordinate; every f32 subtraction p - g is relatively exact, so most errors
// scale with D and are absorbed by rejectBound's factor 1.00001 on the square, i.e. 5e-6 D):
//   the reference's closest point q = a + t ab (or (u a + v b) + w c) is rounded where it is formed: <= 3 u M off the
//     triangle, so its distance may come out that much below the true one                                  1.8e-7 M
//   the record's plane misses the triangle's vertices by e <= 4e-7 of the scale (mesh_tripre_kernel checks) 4.0e-7 M
//   n . (p - g), |p - g|^2 - (n . (p - g))^2, |n| - 1: ~16 u D                                              (factor)
// 2e-6 of the scale is three and a half times their sum.  (Round 2 ran with 2e-5; the margin it adds around every foot
// point, sqrt(2 D slack), was most of what the samples far from the surface queued: a triangle's width and more.)
HPSDF_HD __forceinline__ float meshSlack(const BvhNode& root) {
    float e2 = 0.0f, big = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float hi = fmaxf(root.hi0[a], root.hi1[a]), lo = fminf(root.lo0[a], root.lo1[a]);
        e2 += (hi - lo) * (hi - lo);
        big = fmaxf(big, fmaxf(fabsf(hi), fabsf(lo)));
    }
    return 2e-6f * fmaxf(sqrtf(e2), big);
}
// (closestSimplex's face-case tolerance is MeshDev::faceTolOfSlack of that slack -- a quarter by default: a point it accepts lies at
// most that far outside its triangle, so a distance it returns is at most a quarter of the slack, plus the 3 u M of forming q, below
// the triangle's true distance)
HPSDF_HD __forceinline__ float rejectBound(float best, float slack) {
    const float r = sqrtf(best) + slack;
    return r * r * 1.00001f;
}

// Closest triangle by stack traversal of the device BVH, nearer child first.  Ties on squared distance go to
// the lower triangle index, and a box is pruned only when it is strictly farther than the running best (with a
// guard band for f32 rounding of the box distance), so the winner equals the linear scan of
// Mesh::ClosestTriangleToPt (Mesh.cpp:134-159) whatever the visiting order.  `hint` (the winner of the
// caller's previous, nearby query) is tested first so that the bound is tight from the start.
inline HPSDF_HD float meshSignedDistance(const MeshDev& m, V3 pt, uint32_t& hint) {
    if (!meshPointFinite(pt)) return meshNoTriangle();
    float best = FLT_MAX, reject = __builtin_inff();
    const float slack = meshSlack(m.bvh[0]);
    uint32_t bestTri = 0xFFFFFFFFu;
    int bestCode = 8;
    V3 bestQ = {0.0f, 0.0f, 0.0f};
    auto visitTri = [&](uint32_t t) {
        V3 q;
        const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
        const int code = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, best, q);
        const float d = sqnorm(pt - q);
        if (d < best || (d == best && t < bestTri)) {
            best = d;
            reject = rejectBound(d, slack);
            bestTri = t;
            bestCode = code;
            bestQ = q;
        }
    };
    auto visitLeaf = [&](int32_t c) {
        for (uint32_t k = 0, first = leafFirst(c), cnt = leafCount(c); k < cnt; ++k) {
            const TriPre rec = loadTriPre(m, first + k);
            if (!(triLowerBound2(pt, rec) > reject)) visitTri(triPreTriangle(rec));
        }
    };
    auto boxDist = [&](const float* lo, const float* hi) {
        const float cx = fminf(fmaxf(pt.x, lo[0]), hi[0]);
        const float cy = fminf(fmaxf(pt.y, lo[1]), hi[1]);
        const float cz = fminf(fmaxf(pt.z, lo[2]), hi[2]);
        return sqnorm(pt - V3{cx, cy, cz});
    };
    auto worthIt = [&](float d) { return !(d > best * 1.00001f + 1e-30f); };
    if (hint < m.nTris) visitTri(hint);
    // one deferred sibling per level: the host's median-split tree is <= 31 levels deep, the device's linear BVH (63-bit
    // Morton codes, equal codes split by position) at most 63 + 32
    int32_t stack[96];
    float stackD[96];
    int sp = 0;
    stack[sp] = 0;
    stackD[sp++] = 0.0f;
    while (sp > 0) {
        --sp;
        if (!worthIt(stackD[sp])) continue;  // the bound may have tightened since the push
        const BvhNode n = m.bvh[stack[sp]];
        const float d0 = boxDist(n.lo0, n.hi0), d1 = boxDist(n.lo1, n.hi1);
        // nearer child first; leaves are resolved at once (they tighten the bound for the sibling)
        const bool swap = d1 < d0;
        const int32_t ca = swap ? n.c1 : n.c0, cb = swap ? n.c0 : n.c1;
        const float da = swap ? d1 : d0, db = swap ? d0 : d1;
        int32_t pushA = -1;
        if (worthIt(da)) {
            if (ca < 0)
                visitLeaf(ca);
            else
                pushA = ca;
        }
        if (worthIt(db)) {
            if (cb < 0)
                visitLeaf(cb);
            else if (sp < 95) {
                stack[sp] = cb;
                stackD[sp++] = db;
            }
        }
        if (pushA >= 0 && sp < 96) {  // on top: popped next
            stack[sp] = pushA;
            stackD[sp++] = da;
        }
    }
    if (bestTri == 0xFFFFFFFFu) return meshNoTriangle();  // (every triangle's distance overflowed)
    hint = bestTri;
    const V3 nrm = pseudoNormal(m, bestTri, bestCode);
    const V3 d = pt - bestQ;
    const float sign = dot(nrm, d) > 0.0f ? 1.0f : -1.0f;
    return sign * sqrtf(sqnorm(d));
}

// The same query for the 64 points of a wave at once (the samples of one cell's grid: a tight cluster).  The wave
// walks ONE traversal: a node is visited if any lane still needs it, its 64 bytes are fetched once (every lane reads
// the same address), every lane keeps its own best and tests a triangle only if its own bound asks for it -- so each
// lane ends with exactly what its own traversal finds (pruning is per lane, ties go to the lower triangle index,
// the visiting order does not matter), while the gathers that dominate the per-lane version (64 lanes x dozens of
// scattered 64-byte nodes) become a few dozen uniform loads.  `stack` : kMeshStack ints of LDS owned by this wave (two entries per level of a BVH at most 31 levels deep).
// Every lane of the wave must call this (inactive lanes with active = false).
constexpr int kMeshStack = 128;
inline __device__ float meshSignedDistanceWave(const MeshDev& m, V3 pt, bool activeIn, uint32_t& hint, int32_t* stack) {
    const bool active = activeIn && meshPointFinite(pt);
    float best = FLT_MAX;
    float bound = __builtin_inff();  // best * 1.00001f + 1e-30f, kept beside best: what a box distance is compared with
    float reject = __builtin_inff();  // what a triangle's lower bound is compared with (rejectBound)
    const float slack = meshSlack(m.bvh[0]);
    uint32_t bestTri = 0xFFFFFFFFu;
    int bestCode = 8;
    V3 bestQ = {0.0f, 0.0f, 0.0f};
    auto visitTri = [&](uint32_t t) {
        V3 q;
        const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
        const int code = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, best, q);
        const float d = sqnorm(pt - q);
        if (d < best || (d == best && t < bestTri)) {
            best = d;
            bound = d * 1.00001f + 1e-30f;
            reject = rejectBound(d, slack);
            bestTri = t;
            bestCode = code;
            bestQ = q;
        }
    };
    auto visitLeaf = [&](int32_t c) {
        for (uint32_t k = 0, first = leafFirst(c), cnt = leafCount(c); k < cnt; ++k) {
            const TriPre rec = loadTriPre(m, first + k);
            if (!(triLowerBound2(pt, rec) > reject)) visitTri(triPreTriangle(rec));
        }
    };
    auto boxDist = [&](const float* lo, const float* hi) {  // clamp = median of (p, lo, hi): lo <= hi in every box
        const float cx = __builtin_amdgcn_fmed3f(pt.x, lo[0], hi[0]);
        const float cy = __builtin_amdgcn_fmed3f(pt.y, lo[1], hi[1]);
        const float cz = __builtin_amdgcn_fmed3f(pt.z, lo[2], hi[2]);
        return sqnorm(pt - V3{cx, cy, cz});
    };
    auto worthIt = [&](float d) { return active && !(d > bound); };
    if (active && hint < m.nTris) visitTri(hint);
    const int lane = threadIdx.x & 63;
    // The node being processed lives in registers, the stack only holds the deferred siblings.  Which node comes next is
    // known as soon as the two box tests are in -- the nearer wanted child, else the top of the stack -- so its 64 bytes
    // are asked for BEFORE this node's triangle tests run and arrive behind them (same visiting order as a plain
    // push-both / pop loop; the winner does not depend on the order anyway).
    int sp = 0;  // wave-uniform
#ifdef HPSDF_MESH_STATS_BUILD
    unsigned nVisits = 0, nTriInstr = 0, nTriLanes = 0;
#endif
    BvhNode n = m.bvh[0];
    for (;;) {
#ifdef HPSDF_MESH_STATS_BUILD
        ++nVisits;
#endif
        const float d0 = boxDist(n.lo0, n.hi0), d1 = boxDist(n.lo1, n.hi1);
        const bool w0 = worthIt(d0), w1 = worthIt(d1);
        const unsigned long long b0 = __ballot(w0), b1 = __ballot(w1);
        const int32_t c0 = n.c0, c1 = n.c1;
        int32_t next = -1;
        const bool push0 = c0 >= 0 && b0 != 0ull, push1 = c1 >= 0 && b1 != 0ull;
        if (push0 && push1) {
            // the one that is nearer for the first lane that wants child 0 goes first, its sibling waits on the stack
            const int l0 = __ffsll((long long)b0) - 1;
            const float a0 = __shfl(d0, l0, 64), a1 = __shfl(d1, l0, 64);
            const bool firstIs1 = __builtin_amdgcn_readfirstlane((int)(a1 < a0)) != 0;
            next = firstIs1 ? c1 : c0;
            if (sp < kMeshStack) {
                if (lane == 0) stack[sp] = firstIs1 ? c0 : c1;
                ++sp;
            }
        } else if (push0 || push1) {
            next = push0 ? c0 : c1;
        } else if (sp > 0) {
            --sp;
            next = __builtin_amdgcn_readfirstlane(stack[sp]);
        }
        const BvhNode nn = m.bvh[next >= 0 ? next : 0];  // (the root again when the walk is over: never used)
        // leaves are resolved at once (they tighten the bounds for everything still to come)
        if (c0 < 0 && b0 != 0ull) {
            if (w0) visitLeaf(c0);
#ifdef HPSDF_MESH_STATS_BUILD
            if (m.stats) ++nTriInstr, nTriLanes += (unsigned)__popcll(b0);
#endif
        }
        if (c1 < 0 && b1 != 0ull) {
            if (w1 && worthIt(d1)) visitLeaf(c1);
#ifdef HPSDF_MESH_STATS_BUILD
            if (m.stats) ++nTriInstr, nTriLanes += (unsigned)__popcll(b1);
#endif
        }
        // The test on the two padding words (always zero, mesh.cpp) keeps all sixteen dwords of the prefetch live across
        // the triangle tests: with them dead the register allocator reuses their SGPRs at once and has to wait for the
        // load right where it was issued.  (An empty asm with "s" inputs would do too, but turns every BVH fetch of the
        // kernel into a vector load.)
        if (next < 0 || (nn.pad[0] & nn.pad[1]) == 0xFFFFFFFFu) break;
        n = nn;
    }
#ifdef HPSDF_MESH_STATS_BUILD  // a global atomic in the kernel makes every BVH fetch a vector load: diagnostic builds only
    if (m.stats && lane == 0) {
        atomicAdd(m.stats + 0, 1ull), atomicAdd(m.stats + 1, (unsigned long long)nVisits);
        atomicAdd(m.stats + 2, (unsigned long long)nTriInstr), atomicAdd(m.stats + 3, (unsigned long long)nTriLanes);
    }
#endif
    float r = activeIn ? meshNoTriangle() : 0.0f;
    if (active && bestTri != 0xFFFFFFFFu) {
        hint = bestTri;
        const V3 nrm = pseudoNormal(m, bestTri, bestCode);
        const V3 d = pt - bestQ;
        const float sign = dot(nrm, d) > 0.0f ? 1.0f : -1.0f;
        r = sign * sqrtf(sqnorm(d));
    }
    return r;
}

// A node fetched for the whole wave: the index is wave-uniform and nothing writes the BVH while a kernel walks it, so the
// 64 bytes go through the scalar cache into SGPRs (one s_load_dwordx16) instead of 64 lanes asking the texture path for
// the same line.  The compiler only does that for memory it knows to be invariant -- the constant address space says so;
// through the generic pointer it falls back to four vector loads as soon as the kernel contains an LDS atomic.
__device__ __forceinline__ BvhNode loadNodeUniform(const BvhNode* base, int32_t idx) {
    typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
    const ConstWords w = (ConstWords)(uintptr_t)(base + idx);
    BvhNode n;
    n.lo0[0] = __uint_as_float(w[0]), n.lo0[1] = __uint_as_float(w[1]), n.lo0[2] = __uint_as_float(w[2]);
    n.hi0[0] = __uint_as_float(w[3]), n.hi0[1] = __uint_as_float(w[4]), n.hi0[2] = __uint_as_float(w[5]);
    n.lo1[0] = __uint_as_float(w[6]), n.lo1[1] = __uint_as_float(w[7]), n.lo1[2] = __uint_as_float(w[8]);
    n.hi1[0] = __uint_as_float(w[9]), n.hi1[1] = __uint_as_float(w[10]), n.hi1[2] = __uint_as_float(w[11]);
    n.c0 = (int32_t)w[12], n.c1 = (int32_t)w[13], n.pad[0] = w[14], n.pad[1] = w[15];
    return n;
}

// The same traversal with the triangle tests COMPACTED and FILTERED (what mesh_sample_kernel runs).  In
// meshSignedDistanceWave a leaf is tested the moment it is met, by the lanes whose bound asks for it: ~13 of 64 on a smooth
// 1.3 M-triangle mesh, i.e. the closest-point code runs at a fifth of the machine's width.  Here a leaf only appends one
// (lane, leaf) pair per lane that wants it to ring A in LDS.  Whenever 64 >> leafLog2 pairs are there the wave runs 64
// lower-bound tests at once (triLowerBound2; lane l takes slot l & (W - 1) of pair l >> leafLog2, W = 1 << leafLog2 the most a
// leaf holds; the point comes from its owner's registers by ds_bpermute).  Survivors go to ring B as (lane, triangle);
// whenever 64 are there the wave runs 64 closest-point tests at once and merges every result into its owner's best with ONE
// 64-bit LDS atomic min on (distance bits << 32 | triangle): smallest distance, ties to the lower index -- the linear scan's
// rule (Mesh.cpp:134-159), whatever the order.
// Pruning works on bounds that are refreshed after every closest-point batch: a stale (looser) bound only adds pairs,
// never drops one, so every lane still ends with exactly the triangle its own exhaustive scan finds.  The winner's closest
// point and simplex are recomputed once at the end (same function, same bits).
// Round 3: a child is wanted by a lane only if BOTH its box and its slab (NodeSlab: mesh_build.hip) come within the lane's
// best distance.  A tilted patch of size H fills its box, so by the box alone a sample at distance D wants every patch within
// ~sqrt(D H) of its foot point, at every level of the tree; the slab of a smooth patch is thin and leaves the patches within
// ~H.  The per-lane descent that seeds the bounds follows the smaller of the two children's combined bounds and so ends in
// the leaf under the sample (by boxes alone: a few triangles off, and everything in between passes the lower-bound test).
#ifndef HPSDF_MESH_ABL
#define HPSDF_MESH_ABL 0  // lab builds only (tools/mesh_ablation.sh): what the sampler's phases cost, by leaving one out or running it twice
#endif
constexpr uint32_t kMeshPoolCap = 256;  // (lane, node) pairs a wave's pool holds
#ifndef HPSDF_MESH_SPARSE
#define HPSDF_MESH_SPARSE 16            // a child that at most this many lanes want goes to the pool instead of being walked by the wave
#endif
struct MeshWaveLds {
    unsigned long long best[64];  // per lane: (squared distance bits << 32 | triangle) of the nearest triangle so far
    float px[64], py[64], pz[64]; // per lane: its sample
    float rj[64];                 // per lane: what a lower bound is compared with, rejectBound(best): refreshed with best
    uint32_t nNode[kMeshPoolCap]; // pool N (a stack): (lane, inner node) pairs waiting for their two box / slab tests
    uint32_t aRef[256];           // ring A: (lane, leaf reference) waiting for the lower-bound tests of the leaf's slots
    uint32_t bTri[128];           // ring B: (lane, triangle) waiting for the closest-point test
    int32_t stack[kMeshStack];    // the walk's deferred siblings
    uint8_t nLane[kMeshPoolCap];
    uint8_t aLane[256];
    uint8_t bLane[128];
    uint8_t redo[64];             // lanes whose pairs found the pool full
#ifdef HPSDF_MESH_STALE_STATS
    float bLb[128];               // (diagnostic) ring B: the lower bound each pair passed with
#endif
};
// lower bound of the squared distance from p to anything inside the slab |n . (x - g)| <= e cut by the ball |x - g| <= rho
// (g = (g.xyz), rho = g.w, n = nh.xyz, e = nh.w): along n at least |n . (p - g)| - e, across it at least the distance of p
// from the axis through g minus rho.  Raw v_sqrt_f32 (1 ulp): the caller's slack is four orders of magnitude wider.
__device__ __forceinline__ float slabLowerBound2(V3 p, float4 g, float4 nh) {
    const V3 dx = p - V3{g.x, g.y, g.z};
    const float sd = dotF(V3{nh.x, nh.y, nh.z}, dx);
    const float al = fmaxf(fabsf(sd) - nh.w, 0.0f);
    const float off = fmaxf(__builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-sd, sd, dotF(dx, dx)), 0.0f)) - g.w, 0.0f);
    return __builtin_fmaf(off, off, al * al);
}
__device__ __forceinline__ NodeSlab loadSlabUniform(const NodeSlab* base, int32_t idx) {
    typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
    const ConstWords w = (ConstWords)(uintptr_t)(base + idx);
    NodeSlab s;
    s.g0 = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
    s.n0 = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]), __uint_as_float(w[7]));
    s.g1 = make_float4(__uint_as_float(w[8]), __uint_as_float(w[9]), __uint_as_float(w[10]), __uint_as_float(w[11]));
    s.n1 = make_float4(__uint_as_float(w[12]), __uint_as_float(w[13]), __uint_as_float(w[14]), __uint_as_float(w[15]));
    return s;
}
inline __device__ float meshSignedDistanceWaveQ(const MeshDev& m, V3 pt, bool activeIn, MeshWaveLds& L) {
    const bool active = activeIn && meshPointFinite(pt);
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    L.best[lane] = ((unsigned long long)__float_as_uint(FLT_MAX) << 32) | 0xFFFFFFFFull;
    L.px[lane] = pt.x, L.py[lane] = pt.y, L.pz[lane] = pt.z;
    L.redo[lane] = 0;
    uint32_t nCount = 0, aHead = 0, aCount = 0, bHead = 0, bCount = 0;  // wave-uniform
    float bound = __builtin_inff();   // what a box distance is compared with: best * 1.00001f + 1e-30f
    float reject = __builtin_inff();  // what a lower bound is compared with: rejectBound(best)
    const uint32_t lg = m.leafLog2, perBatch = 64u >> lg;               // pairs of ring A one lower-bound batch takes
    const bool slabs = m.slabs != nullptr;
    const uint32_t poolCap = m.poolCap < 128u ? 128u : (m.poolCap > kMeshPoolCap ? kMeshPoolCap : m.poolCap);
    const float inf = __builtin_inff();
#ifdef HPSDF_MESH_STATS_BUILD
    unsigned nVisits = 0, nBound = 0, nClosest = 0;  // [1] nodes visited, [2] pairs through the lower-bound test, [3] through the closest-point test
    unsigned nPairs = 0, nBoundBatches = 0, nClosestBatches = 0, nSeedExact = 0;  // [4] (lane, leaf) pairs, [5] [6] batches, [7] lanes whose seed was the answer
    float seedBest = 0.0f;
    unsigned nPoolPairs = 0;
#endif
    const float slack = meshSlack(loadNodeUniform(m.bvh, 0));
    // the owner's sample and bounds as the batches see them: always the latest best (the closest-point batches write it)
    auto ownerPoint = [&](int o) { return V3{L.px[o], L.py[o], L.pz[o]}; };
    auto ownerBest = [&](int o) { return __uint_as_float((uint32_t)(L.best[o] >> 32)); };
    auto closestBatch = [&](uint32_t cnt) {  // the first cnt (<= 64) pairs of ring B
        const bool on = (uint32_t)lane < cnt;
        const uint32_t at = (bHead + (uint32_t)lane) & 127u;
        const uint32_t t = on ? L.bTri[at] : 0u;
        const int src = on ? (int)L.bLane[at] : lane;
        const V3 p = ownerPoint(src);
#ifdef HPSDF_MESH_STALE_STATS  // [7]: pairs whose bound no longer passes when their closest-point test runs (the owner's best has improved since)
        nSeedExact += (unsigned)__popcll(__ballot(on && L.bLb[at] > L.rj[src]));
#endif
        if (on) {
            V3 q;
            const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
            closestSimplex(p, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, ownerBest(src), q);  // (a stale best only substitutes more often than needed)
            const float d = sqnorm(p - q);
            atomicMin(&L.best[src], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)t);
#if HPSDF_MESH_ABL == 5  // (lab: the closest-point test twice -- what the batches cost is the difference)
            {
                V3 p2 = p, q2;
                asm volatile("" : "+v"(p2.x));
                closestSimplex(p2, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, ownerBest(src), q2);
                const float d2 = sqnorm(p2 - q2);
                asm volatile("" ::"v"(d2));
            }
#endif
        }
        __builtin_amdgcn_wave_barrier();
        const float best = ownerBest(lane);
        bound = best * 1.00001f + 1e-30f;
        reject = rejectBound(best, slack);
        L.rj[lane] = reject;
        bHead = (bHead + cnt) & 127u;
        bCount -= cnt;
#ifdef HPSDF_MESH_STATS_BUILD
        nClosest += cnt;
#ifndef HPSDF_MESH_VISIT_HIST
        ++nClosestBatches;
#endif
#endif
    };
    auto boundBatch = [&](uint32_t pairs) {  // the first `pairs` (<= perBatch) pairs of ring A; ring B holds < 64 on entry
        const uint32_t e = (uint32_t)lane >> lg, k = (uint32_t)lane & ((1u << lg) - 1u);
        const uint32_t at = (aHead + e) & 255u;
        const bool have = e < pairs;
        const int32_t ref = have ? (int32_t)L.aRef[at] : -1;
        const int src = have ? (int)L.aLane[at] : lane;
        const bool on = have && k < leafCount(ref);
        const uint32_t slot = leafFirst(ref) + k;
        const V3 p = ownerPoint(src);
        const float rj = L.rj[src];
        bool pass = false;
        uint32_t tri = 0u;
        float lbv = 0.0f;
        if (on) {
            const TriPre rec = loadTriPre(m, slot);
            tri = triPreTriangle(rec);
            lbv = triLowerBound2(p, rec);
            pass = !(lbv > rj);  // (a NaN passes)
#if HPSDF_MESH_ABL == 6  // (lab: the lower-bound test twice)
            {
                V3 p2 = p;
                asm volatile("" : "+v"(p2.x));
                const float lb2 = triLowerBound2(p2, rec);
                asm volatile("" ::"v"(lb2));
            }
#endif
        }
        const unsigned long long pb = __ballot(pass);
        if (pass) {
            const uint32_t pos = (bHead + bCount + (uint32_t)__popcll(pb & below)) & 127u;
            L.bTri[pos] = tri;
            L.bLane[pos] = (uint8_t)src;
#ifdef HPSDF_MESH_STALE_STATS
            L.bLb[pos] = lbv;
#endif
        }
        bCount += (uint32_t)__popcll(pb);
        aHead = (aHead + pairs) & 255u;
        aCount -= pairs;
#ifdef HPSDF_MESH_STATS_BUILD
        nBound += (unsigned)__popcll(__ballot(on));
#ifndef HPSDF_MESH_VISIT_HIST
        ++nBoundBatches;
#endif
#endif
        __builtin_amdgcn_wave_barrier();
        while (bCount >= 64) closestBatch(64);
    };
    auto boxDist6 = [&](V3 p, float lx, float ly, float lz, float hx, float hy, float hz) {  // clamp = median of (p, lo, hi): lo <= hi in every box
        const float cx = __builtin_amdgcn_fmed3f(p.x, lx, hx);
        const float cy = __builtin_amdgcn_fmed3f(p.y, ly, hy);
        const float cz = __builtin_amdgcn_fmed3f(p.z, lz, hz);
        const V3 dd = p - V3{cx, cy, cz};
        return dotF(dd, dd);
    };
#define HPSDF_BOX0(p, nd) boxDist6(p, (nd).lo0[0], (nd).lo0[1], (nd).lo0[2], (nd).hi0[0], (nd).hi0[1], (nd).hi0[2])
#define HPSDF_BOX1(p, nd) boxDist6(p, (nd).lo1[0], (nd).lo1[1], (nd).lo1[2], (nd).hi1[0], (nd).hi1[1], (nd).hi1[2])
    // Seeds.  Everything the walk below queues for a lane is what lies within the lane's best distance so far, and a best
    // that is off by a fraction f of the distance D admits everything within sqrt(2 f) D of the foot point: 1 % is already
    // 0.14 D, a dozen triangles across on a fine mesh.  So before anything is queued every lane gets a best distance that is
    // the final one for most samples, in three steps (HPSDF_MESH_STATS_BUILD counts how many):
    //   1. it walks down to ONE leaf of its own, towards the child whose centre is nearer (lower bounds decide badly here:
    //      a sample sits inside both children's balls and slabs half of the time, and then their tilt decides), and tests
    //      the leaf's triangles, the one with the smallest lower bound first, the others only if their bound allows;
    //   2. it tries the triangles its six neighbours in the wave's 4 x 4 x 4 block of samples ended with, if their lower
    //      bound allows, nearest bound first (a descent that took a wrong turn high up ends several leaves away; the
    //      neighbouring sample's, three triangles further on, most likely did not) -- twice;
    //   3. it walks over the mesh: while the closest point lies on an edge (or corner) of its triangle, the triangle across
    //      that edge is tried -- the distance falls with every step, and the walk ends on the foot point's triangle unless
    //      the surface folds in between.
    // None of this has to be right: the walk below finds whatever is nearer.
#ifndef HPSDF_SEED_EXCHANGE
#define HPSDF_SEED_EXCHANGE 2
#endif
#ifndef HPSDF_SEED_WALK
#define HPSDF_SEED_WALK 6
#endif
    {
        float best = FLT_MAX, rj = inf;
        uint32_t bestTri = 0xFFFFFFFFu, bestSlot = 0xFFFFFFFFu;
        int bestCode = 8;
        auto tryTriangle = [&](uint32_t t, uint32_t slot) {
            V3 q;
            const float4 tp[3] = {m.triPos[3 * (size_t)t], m.triPos[3 * (size_t)t + 1], m.triPos[3 * (size_t)t + 2]};
            const int code = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, best, q);
            const float d = sqnorm(pt - q);
            const bool better = d < best || (d == best && t < bestTri);
            if (better) best = d, bestTri = t, bestSlot = slot, bestCode = code, rj = rejectBound(d, slack);
            return better;
        };
        uint32_t restMask = 0u, seedFirst = 0u;
        if (active) {
            int32_t c = 0;
            do {
                const BvhNode nd = m.bvh[c];
                bool second;
                if (slabs) {
                    const NodeSlab ns = m.slabs[c];
                    second = sqnorm(pt - V3{ns.g1.x, ns.g1.y, ns.g1.z}) < sqnorm(pt - V3{ns.g0.x, ns.g0.y, ns.g0.z});
                } else {
                    second = HPSDF_BOX1(pt, nd) < HPSDF_BOX0(pt, nd);
                }
                c = second ? nd.c1 : nd.c0;
            } while (c >= 0);
            const uint32_t first = leafFirst(c), cnt = leafCount(c);
            seedFirst = first;
            uint32_t kMin = 0;
            float lbMin = inf;
            for (uint32_t k = 0; k < cnt; ++k) {
                const float lb = triLowerBound2(pt, loadTriPre(m, first + k));
                if (lb < lbMin) lbMin = lb, kMin = k;
            }
            tryTriangle(slotTriangle(m, first + kMin), first + kMin);
            uint32_t rest = 0;  // the other slots whose bound the first test's distance allows
            for (uint32_t k = 0; k < cnt; ++k)
                if (k != kMin && !(triLowerBound2(pt, loadTriPre(m, first + k)) > rj)) rest |= 1u << k;
            restMask = rest;
        }
        // (the remaining candidates of all lanes side by side: as many rounds as the lane with the most of them has -- two or
        // three -- instead of one round per slot of the leaf)
        while (__ballot(restMask != 0u) != 0ull) {
            if (restMask != 0u) {
                const uint32_t k = (uint32_t)__ffs((int)restMask) - 1u;
                restMask &= restMask - 1u;
                const TriPre rec = loadTriPre(m, seedFirst + k);
                if (!(triLowerBound2(pt, rec) > rj)) tryTriangle(triPreTriangle(rec), seedFirst + k);
            }
        }
        for (int pass = 0; pass < HPSDF_SEED_EXCHANGE; ++pass) {
            uint32_t candSlot = 0xFFFFFFFFu, candTri = 0u;
            float candLb = inf;
#pragma unroll
            for (int nb = 0; nb < 6; ++nb) {
                const int off = nb < 2 ? 1 : (nb < 4 ? 4 : 16);
                const int src = (lane + ((nb & 1) ? off : 64 - off)) & 63;
                const uint32_t slot = (uint32_t)__shfl((int)bestSlot, src, 64);
                if (active && slot != 0xFFFFFFFFu && slot != bestSlot) {
                    const TriPre rec = loadTriPre(m, slot);
                    const float lb = triLowerBound2(pt, rec);
                    if (lb < candLb && !(lb > rj)) candLb = lb, candSlot = slot, candTri = triPreTriangle(rec);
                }
            }
            if (candSlot != 0xFFFFFFFFu) tryTriangle(candTri, candSlot);
        }
        {
            // (one triangle per lane and step: at a corner the edge that starts there first, and if that does not help the
            // edge that ends there in the next step)
            bool moving = active;
            int second = -1;  // the other edge of a corner whose first edge did not help
            for (int step = 0; step < HPSDF_SEED_WALK && __ballot(moving) != 0ull; ++step) {
                if (moving) {
                    int e = second;
                    second = -1;
                    if (e < 0 && bestCode != 8) {
                        e = bestCode >= 4 ? bestCode - 4 : bestCode;
                        if (bestCode < 4) second = (bestCode + 2) % 3;
                    }
                    moving = false;
                    if (e >= 0) {
                        const uint32_t t = m.halfEdges[3 * bestTri + (uint32_t)e] / 3u;
                        if (tryTriangle(t, 0xFFFFFFFFu))
                            moving = true, second = -1;
                        else
                            moving = second >= 0;
                    }
                }
            }
        }
        if (active) {
            L.best[lane] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)bestTri;
            bound = best * 1.00001f + 1e-30f;
            reject = rj;
        }
        L.rj[lane] = reject;
#ifdef HPSDF_MESH_STATS_BUILD
        seedBest = best;
#endif
    }
    __builtin_amdgcn_wave_barrier();
    // The walk: the wave visits a node if any lane still wants it, every lane against its own bound -- as long as MANY lanes
    // want it.  High up every lane wants the same few nodes and a visit (one 128-byte fetch through the scalar cache, two
    // box and two slab tests across the wave) serves them all; near the leaves the samples' foot points lie a dozen triangles
    // apart, half of the visits serve four lanes or fewer, and the wave-wide tests run for them alone.  So a child that at
    // most HPSDF_MESH_SPARSE lanes want is not walked: each of those lanes drops a (lane, node) pair into a pool in LDS, and
    // whenever 64 pairs are there one batch tests 64 pairs at once -- lane l fetches ITS pair's node and slab, tests both
    // children for the pair's owner (whose sample and bounds come from LDS), inner children that pass go back into the pool
    // (the nearer one on top), leaf children to ring A.  (The pool for EVERYTHING, from the root, was tried first: a lane
    // wants ~170 nodes, 30 lanes share a node on average, and the pool moved 1.4 MB of nodes per wave through the vector
    // memory path where the walk moves 45 KB through the scalar cache -- 10.1 against 7.1 ms.)  Every pair is tested against
    // its owner's own bound, so each lane still ends with exactly what its own exhaustive scan finds.  If the pool is ever
    // full, the owners concerned are marked and walk the tree once more at the end, without a pool.
    auto poolBatch = [&]() {
        const uint32_t cnt = nCount < 64u ? nCount : 64u;
        const bool on = (uint32_t)lane < cnt;
        const uint32_t at = on ? nCount - 1u - (uint32_t)lane : 0u;  // lane 0 takes the top of the stack
        const uint32_t node = on ? L.nNode[at] : 0u;
        const int o = on ? (int)L.nLane[at] : lane;
        nCount -= cnt;
        const V3 p = ownerPoint(o);
        const float bd = ownerBest(o) * 1.00001f + 1e-30f, rj = L.rj[o];
        bool w0 = false, w1 = false;
        int32_t c0 = 0, c1 = 0;
        float k0 = 0.0f, k1 = 0.0f;
        if (on) {
            const BvhNode nd = m.bvh[node];
            k0 = HPSDF_BOX0(p, nd), k1 = HPSDF_BOX1(p, nd);
            w0 = !(k0 > bd), w1 = !(k1 > bd);
            c0 = nd.c0, c1 = nd.c1;
            if (slabs) {
                const NodeSlab ns = m.slabs[node];
                if (ns.n0.w >= 0.0f) {
                    const float sb = slabLowerBound2(p, ns.g0, ns.n0);
                    w0 = w0 && !(sb > rj), k0 = fmaxf(k0, sb);
                }
                if (ns.n1.w >= 0.0f) {
                    const float sb = slabLowerBound2(p, ns.g1, ns.n1);
                    w1 = w1 && !(sb > rj), k1 = fmaxf(k1, sb);
                }
            }
        }
#ifdef HPSDF_MESH_STATS_BUILD
        nPoolPairs += cnt;
#endif
        const bool i0 = w0 && c0 >= 0, i1 = w1 && c1 >= 0, l0 = w0 && c0 < 0, l1 = w1 && c1 < 0;
        {   // inner children back to the pool: the farther one first, so that the nearer one is popped first
            const unsigned long long bAny = __ballot(i0 || i1), bTwo = __ballot(i0 && i1);
            const uint32_t total = (uint32_t)(__popcll(bAny) + __popcll(bTwo));
            if (nCount + total <= poolCap) {
                if (i0 || i1) {
                    const uint32_t pos = nCount + (uint32_t)(__popcll(bAny & below) + __popcll(bTwo & below));
                    const bool both = i0 && i1, nearIs1 = k1 < k0;
                    L.nNode[pos] = (uint32_t)(both ? (nearIs1 ? c0 : c1) : (i0 ? c0 : c1));
                    L.nLane[pos] = (uint8_t)o;
                    if (both) {
                        L.nNode[pos + 1u] = (uint32_t)(nearIs1 ? c1 : c0);
                        L.nLane[pos + 1u] = (uint8_t)o;
                    }
                }
                nCount += total;
            } else if (i0 || i1) {
                L.redo[o] = 1;  // no room: this owner walks the tree again at the end
            }
        }
        {   // leaf children to ring A (which holds < perBatch on entry: at most 63 + 128 of its 256)
            const unsigned long long bAny = __ballot(l0 || l1), bTwo = __ballot(l0 && l1);
            if (l0 || l1) {
                const uint32_t pos = aHead + aCount + (uint32_t)(__popcll(bAny & below) + __popcll(bTwo & below));
                L.aRef[pos & 255u] = (uint32_t)(l0 ? c0 : c1);
                L.aLane[pos & 255u] = (uint8_t)o;
                if (l0 && l1) {
                    L.aRef[(pos + 1u) & 255u] = (uint32_t)c1;
                    L.aLane[(pos + 1u) & 255u] = (uint8_t)o;
                }
            }
            aCount += (uint32_t)(__popcll(bAny) + __popcll(bTwo));
#if defined(HPSDF_MESH_STATS_BUILD) && !defined(HPSDF_MESH_VISIT_HIST)
            nPairs += (unsigned)(__popcll(bAny) + __popcll(bTwo));
#endif
        }
        __builtin_amdgcn_wave_barrier();
        while (aCount >= perBatch) boundBatch(perBatch);
    };
    auto walk = [&](bool act, uint32_t sparse) {  // sparse = 0: no pool, the wave walks everything some lane wants
        BvhNode n = loadNodeUniform(m.bvh, 0);
        NodeSlab sl{};
        if (slabs) sl = loadSlabUniform(m.slabs, 0);
        int sp = 0;  // wave-uniform
        for (;;) {
#ifdef HPSDF_MESH_STATS_BUILD
            ++nVisits;
#endif
            const float d0 = HPSDF_BOX0(pt, n), d1 = HPSDF_BOX1(pt, n);
            bool w0 = act && !(d0 > bound), w1 = act && !(d1 > bound);
            if (slabs) {  // (wave-uniform conditions: the slab came through the scalar cache)
                if (sl.n0.w >= 0.0f && __ballot(w0) != 0ull) w0 = w0 && !(slabLowerBound2(pt, sl.g0, sl.n0) > reject);
                if (sl.n1.w >= 0.0f && __ballot(w1) != 0ull) w1 = w1 && !(slabLowerBound2(pt, sl.g1, sl.n1) > reject);
            }
            const unsigned long long b0 = __ballot(w0), b1 = __ballot(w1);
            const int32_t c0 = n.c0, c1 = n.c1;
#ifdef HPSDF_MESH_VISIT_HIST  // how many lanes a visit serves: [4] <= 4 lanes wanted one of the children, [5] <= 8, [6] <= 16, [7] <= 32
            {
                const int pc = __popcll(b0 | b1);
                nPairs += pc <= 4 ? 1u : 0u, nBoundBatches += pc > 4 && pc <= 8 ? 1u : 0u, nClosestBatches += pc > 8 && pc <= 16 ? 1u : 0u;
                nSeedExact += pc > 16 && pc <= 32 ? 1u : 0u;
            }
#endif
            bool push0 = c0 >= 0 && b0 != 0ull, push1 = c1 >= 0 && b1 != 0ull;
            // inner children few lanes want: into the pool (if it has room for them and for what a batch can add)
            if (push0 && (uint32_t)__popcll(b0) <= sparse && nCount + (uint32_t)__popcll(b0) + 64u <= poolCap) {
                if (w0) {
                    const uint32_t pos = nCount + (uint32_t)__popcll(b0 & below);
                    L.nNode[pos] = (uint32_t)c0;
                    L.nLane[pos] = (uint8_t)lane;
                }
                nCount += (uint32_t)__popcll(b0);
                push0 = false;
            }
            if (push1 && (uint32_t)__popcll(b1) <= sparse && nCount + (uint32_t)__popcll(b1) + 64u <= poolCap) {
                if (w1) {
                    const uint32_t pos = nCount + (uint32_t)__popcll(b1 & below);
                    L.nNode[pos] = (uint32_t)c1;
                    L.nLane[pos] = (uint8_t)lane;
                }
                nCount += (uint32_t)__popcll(b1);
                push1 = false;
            }
            int32_t next = -1;
            if (push0 && push1) {
                // the one that is nearer for the first lane that wants child 0 goes first, its sibling waits on the stack
                const int l0 = __ffsll((long long)b0) - 1;
                const float a0 = __shfl(d0, l0, 64), a1 = __shfl(d1, l0, 64);
                const bool firstIs1 = __builtin_amdgcn_readfirstlane((int)(a1 < a0)) != 0;
                next = firstIs1 ? c1 : c0;
                if (sp < kMeshStack) {
                    if (lane == 0) L.stack[sp] = firstIs1 ? c0 : c1;
                    ++sp;
                }
            } else if (push0 || push1) {
                next = push0 ? c0 : c1;
            } else if (sp > 0) {
                --sp;
                next = __builtin_amdgcn_readfirstlane(L.stack[sp]);
            }
            // the next node's 128 bytes are asked for before this node's leaves are queued and tested
            const int32_t nextIdx = __builtin_amdgcn_readfirstlane(next >= 0 ? next : 0);  // (the root again when the walk is over: never used)
            const BvhNode nn = loadNodeUniform(m.bvh, nextIdx);
            NodeSlab sn{};
            if (slabs) sn = loadSlabUniform(m.slabs, nextIdx);
            for (int side = 0; side < 2; ++side) {  // leaves: one (lane, leaf) pair per lane that wants it
                const int32_t c = side ? c1 : c0;
                const unsigned long long b = side ? b1 : b0;
                if (c >= 0 || b == 0ull) continue;
                if (side ? w1 : w0) {
                    const uint32_t pos = (aHead + aCount + (uint32_t)__popcll(b & below)) & 255u;
                    L.aRef[pos] = (uint32_t)c;
                    L.aLane[pos] = (uint8_t)lane;
                }
                aCount += (uint32_t)__popcll(b);
#if defined(HPSDF_MESH_STATS_BUILD) && !defined(HPSDF_MESH_VISIT_HIST)
                nPairs += (unsigned)__popcll(b);
#endif
                __builtin_amdgcn_wave_barrier();
                while (aCount >= perBatch) boundBatch(perBatch);
            }
            __builtin_amdgcn_wave_barrier();
            while (nCount >= 64u) poolBatch();
            // (the test on the two padding words, always zero, keeps all sixteen dwords of the prefetch live across the
            // leaf tests: with them dead the register allocator reuses their SGPRs at once and waits for the load right here)
            if (next < 0 || (nn.pad[0] & nn.pad[1]) == 0xFFFFFFFFu) break;
            n = nn;
            sl = sn;
        }
        while (nCount > 0u) poolBatch();
        while (aCount) boundBatch(aCount < perBatch ? aCount : perBatch);
        if (bCount) closestBatch(bCount);
    };
#if HPSDF_MESH_ABL != 2  // (lab 2: seeds only)
    walk(active, (uint32_t)HPSDF_MESH_SPARSE);
    {
        const bool again = L.redo[lane] != 0;
        if (__ballot(again) != 0ull) walk(again, 0u);
    }
#endif
#ifdef HPSDF_MESH_STATS_BUILD
#ifndef HPSDF_MESH_VISIT_HIST
#ifndef HPSDF_MESH_STALE_STATS
    nSeedExact = (unsigned)__popcll(__ballot(active && seedBest == ownerBest(lane)));
#endif
#endif
#ifdef HPSDF_MESH_POOL_STATS  // [7]: (lane, node) pairs that went through the pool
    nSeedExact = nPoolPairs;
#endif
#ifdef HPSDF_MESH_SEED_STATS  // how far off the seeds are: [5] within 1e-4 of the final distance, [6] within 1e-2, [4] within 10 %
    {
        const float rs = sqrtf(seedBest), rf = sqrtf(ownerBest(lane));
        nBoundBatches = (unsigned)__popcll(__ballot(active && rs <= rf * 1.0001f));
        nClosestBatches = (unsigned)__popcll(__ballot(active && rs <= rf * 1.01f));
        nPairs = (unsigned)__popcll(__ballot(active && rs <= rf * 1.1f));
    }
#endif
    if (m.stats && lane == 0) {
        atomicAdd(m.stats + 0, 1ull), atomicAdd(m.stats + 1, (unsigned long long)nVisits);
        atomicAdd(m.stats + 2, (unsigned long long)nBound), atomicAdd(m.stats + 3, (unsigned long long)nClosest);
        atomicAdd(m.stats + 4, (unsigned long long)nPairs), atomicAdd(m.stats + 5, (unsigned long long)nBoundBatches);
        atomicAdd(m.stats + 6, (unsigned long long)nClosestBatches), atomicAdd(m.stats + 7, (unsigned long long)nSeedExact);
    }
#endif
    float r = activeIn ? meshNoTriangle() : 0.0f;
    if (active && (uint32_t)(L.best[lane] & 0xFFFFFFFFull) != 0xFFFFFFFFu) {
        const uint32_t bestTri = (uint32_t)(L.best[lane] & 0xFFFFFFFFull);
        V3 bestQ;
        const float4 tp[3] = {m.triPos[3 * (size_t)bestTri], m.triPos[3 * (size_t)bestTri + 1], m.triPos[3 * (size_t)bestTri + 2]};
#if HPSDF_MESH_ABL == 1  // (lab: no recomputation of the winner's closest point, no pseudo-normal)
        (void)tp, (void)bestQ;
        r = sqrtf(ownerBest(lane));
#elif HPSDF_MESH_ABL == 9  // (lab: the closest point, but the face normal for every case)
        const int bestCode = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, __builtin_inff(), bestQ);
        (void)bestCode;
        const V3 nrm = pseudoNormal(m, bestTri, 8);
        const V3 d = pt - bestQ;
        const float sign = dot(nrm, d) > 0.0f ? 1.0f : -1.0f;
        r = sign * sqrtf(sqnorm(d));
#else
        const int bestCode = closestSimplex(pt, V3{tp[0].x, tp[0].y, tp[0].z}, V3{tp[0].w, tp[1].x, tp[1].y}, V3{tp[1].z, tp[1].w, tp[2].x}, V3{tp[2].y, tp[2].z, tp[2].w}, m.faceTolOfSlack * slack, __builtin_inff(), bestQ);
        const V3 nrm = pseudoNormal(m, bestTri, bestCode);
        const V3 d = pt - bestQ;
        const float sign = dot(nrm, d) > 0.0f ? 1.0f : -1.0f;
        r = sign * sqrtf(sqnorm(d));
#endif
    }
    return r;
}
#undef HPSDF_BOX0
#undef HPSDF_BOX1

// Mesh fields: the order in which the np x nq x nq samples of a chunk are handed to the lanes.  A wave answers its 64
// closest-triangle queries with ONE traversal whose cost is the union of what its lanes need, so the 64 samples should
// sit close together: the chunk is cut into 4 x 4 x 4 blocks (smaller at the upper edges), blocks in (i, j, k) order,
// samples inside a block likewise -- in SPACE, not in index: the Gauss-Legendre tables list their roots as 0, -a, +a, ...
// (Legendre.h), so posI / posJK map a position along the axis (ascending coordinate) to the root's index (posI: among
// the chunk's np planes).  Returns the sample (il * nq + j) * nq + k that position r of that order holds.
// Every sample's value is independent of its companions (pruning is per lane), so this is a pure scheduling choice.
__device__ __forceinline__ int meshSampleOrder(int r, int np, int nq, const unsigned char* posI, const unsigned char* posJK) {
    const int nq2 = nq * nq;
    const int nbi = (np + 3) >> 2, nbj = (nq + 3) >> 2;
    int bi = min(r / (4 * nq2), nbi - 1);
    r -= bi * 4 * nq2;
    const int di = min(4, np - 4 * bi);
    const int strip = di * 4 * nq;
    int bj = min(r / strip, nbj - 1);
    r -= bj * strip;
    const int dj = min(4, nq - 4 * bj);
    const int blk = di * dj * 4;
    int bk = min(r / blk, nbj - 1);
    r -= bk * blk;
    const int dk = min(4, nq - 4 * bk);
    const int a = r / (dj * dk), rest = r - a * (dj * dk), b = rest / dk, c = rest - b * dk;
    return ((int)posI[4 * bi + a] * nq + (int)posJK[4 * bj + b]) * nq + (int)posJK[4 * bk + c];
}

}  // namespace hpsdf
