"""A checker of the data a mesh field's traversals prune by, in numpy float64: the arrays Field.mesh_arrays() exports (BVH nodes with
both children's boxes, slabs, triPre records, triPos, twins) against the mesh itself.  Written from the layout comments of
csrc/device_types.hpp and the invariants the kernels document; it calls nothing from the product.

Every check returns a list of offenders (tuples that start with the node or slot number), empty when the invariant holds; a test
asserts `not offenders` and prints the first few.  A check leaves out what an upstream check already reports (a leaf whose run overlaps
its neighbour's is not also reported as a box that does not contain its triangles): every defect has ONE owner, which
tests/test_mesh_structure_cpu.py proves mutation by mutation.

Work is vectorised per tree level.  The walk lays the leaf runs out in depth-first order ("traversal order"), in which every subtree's
slots are one contiguous range whatever the builder did (the device build's slot ranges are contiguous anyway, the host build's
one-triangle leaves are not): reductions over a child's triangles are np.ufunc.reduceat over that order, node x vertex rows np.repeat.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from helpers import closest_point_on_triangle_f64

LEAF_SHIFT = 4                 # device_types.hpp: kMeshLeafShift
POINT_STACK_DEPTH = 95         # mesh_distance.hpp, meshSignedDistance: one deferred sibling per level, 96 entries
WAVE_STACK = 128               # mesh_distance.hpp: kMeshStack
SLAB_MAX_TRIS = 131072         # mesh_build.hip: HPSDF_SLAB_MAX_TRIS
FRAME_TOL = 1e-6               # mesh_tripre_kernel, mbChildSlab: how far from orthonormal a stored frame may be (|n|^2, |u|^2, n . u)
BOUND_SHARE_OF_SLACK = 0.5     # what a lower bound may exceed the true distance by, as a fraction of the slack (see check_bounds)
_THREADS = 8
_CHUNK_ROWS = 81920         # (point, triangle) pairs per closest-point pass
# one 64-byte BvhNode / NodeSlab (csrc/device_types.hpp), as the export returns them
BVH_DTYPE = np.dtype([("lo0", np.float32, 3), ("hi0", np.float32, 3), ("lo1", np.float32, 3), ("hi1", np.float32, 3),
                      ("c0", np.int32), ("c1", np.int32), ("pad", np.uint32, 2)])
SLAB_DTYPE = np.dtype([("g0", np.float32, 4), ("n0", np.float32, 4), ("g1", np.float32, 4), ("n1", np.float32, 4)])


def first(offenders, n=5):
    """What an assertion message shows: how many and the first few."""
    return "%d offenders, first: %r" % (len(offenders), offenders[:n])


def mesh_scale(verts):
    """meshSlack's scale, restated from its comment: the extent's diagonal, or the largest coordinate if that is larger."""
    v = np.asarray(verts, np.float64)
    return max(float(np.linalg.norm(v.max(0) - v.min(0))), float(np.abs(v).max()))


def mesh_slack(verts):
    return 2e-6 * mesh_scale(verts)


# ------------------------------------------------------------------------------------------------------------------ the walk
class Walk:
    """The children the traversal can reach from node 0, one ENTRY per (node, side), in breadth-first order (the two sides of a node
    adjacent): node, side, ref (BvhNode::c0 / c1), level (depth of the node: the root's is 0), parent (the entry of the node itself,
    -1 for the root's), child0 (the entry of an inner child's side 0, -1 for leaves), defer (nodes on the path, this one included,
    whose children are both inner: what the shared walk has deferred at most when it is here), first / count of leaf runs, size
    (slots below), off (where they start in traversal order), ok (nothing below is reported by check_shape), and `order`: the slot at
    every traversal position."""


def _seg_reduce(ufunc, x, start, size):
    """ufunc over x[start[i] : start[i] + size[i]] along axis 0 for every i (size >= 1)."""
    pad = np.concatenate([x, x[-1:]]) if len(x) else x
    idx = np.empty(2 * len(start), np.int64)
    idx[0::2], idx[1::2] = start, start + size
    return ufunc.reduceat(pad, idx, axis=0)[0::2]


def walk(arr):
    bvh, n_nodes, n_tris = arr["bvh"], len(arr["bvh"]), int(arr["nTris"])
    c = np.stack([bvh["c0"], bvh["c1"]], 1).astype(np.int64)
    w = Walk()
    cols = {k: [] for k in ("node", "side", "ref", "level", "parent", "defer")}
    w.bad_ref, w.twice = [], []
    visited = np.zeros(n_nodes, bool)
    visited[0] = True
    frontier, f_parent, f_defer = np.array([0]), np.array([-1]), np.array([0])
    level = base = 0
    while frontier.size:
        refs = c[frontier].reshape(-1)
        nodes, sides = np.repeat(frontier, 2), np.tile([0, 1], len(frontier))
        defer = np.repeat(f_defer + (c[frontier] >= 0).all(1), 2)
        for k, v in (("node", nodes), ("side", sides), ("ref", refs), ("level", np.full(len(refs), level)),
                     ("parent", np.repeat(f_parent, 2)), ("defer", defer)):
            cols[k].append(v)
        idx = base + np.arange(len(refs))
        inner = refs >= 0
        oob = inner & (refs >= n_nodes)
        w.bad_ref += [(int(a), int(b), int(r)) for a, b, r in zip(nodes[oob], sides[oob], refs[oob])]
        cand = inner & ~oob
        r, ci, cd = refs[cand], idx[cand], defer[cand]
        again = visited[r].copy()
        dup = np.ones(len(r), bool)
        dup[np.unique(r, return_index=True)[1]] = False
        again |= dup
        w.twice += [(int(nodes[cand][i]), int(sides[cand][i]), int(r[i])) for i in np.nonzero(again)[0]]
        frontier, f_parent, f_defer = r[~again], ci[~again], cd[~again]
        visited[frontier] = True
        base += len(refs)
        level += 1
    for k, v in cols.items():
        setattr(w, k, np.concatenate(v))
    w.n = n = len(w.ref)
    w.depth = level - 1  # of the deepest reachable node
    w.visited = visited
    w.child0 = np.full(n, -1, np.int64)
    kids = np.nonzero((w.parent >= 0) & (w.side == 0))[0]
    w.child0[w.parent[kids]] = kids
    # leaf runs
    w.leaf = w.ref < 0
    code = ~w.ref
    w.first = np.where(w.leaf, code >> LEAF_SHIFT, 0)
    w.count = np.where(w.leaf, (code & ((1 << LEAF_SHIFT) - 1)) + 1, 0)
    w.leaf_log2 = int(arr["leafLog2"])
    w.bad_run = w.leaf & ((w.count > (1 << w.leaf_log2)) | (w.first + w.count > n_tris))
    lo, hi = np.minimum(w.first, n_tris), np.minimum(w.first + w.count, n_tris)  # (clipped: what the arrays hold)
    cover = np.zeros(n_tris + 1, np.int64)
    np.add.at(cover, lo[w.leaf], 1)
    np.add.at(cover, hi[w.leaf], -1)
    w.cover = np.cumsum(cover)[:n_tris]
    w.first, w.count = lo, hi - lo
    shared = _seg_reduce(np.maximum, w.cover, np.minimum(w.first, max(n_tris - 1, 0)), np.maximum(w.count, 1)) > 1
    w.overlap = w.leaf & (w.count > 0) & shared
    # the triangle of every slot
    w.slot_tri = np.ascontiguousarray(arr["triPre"][:, 11]).view(np.uint32).astype(np.int64)
    seen = np.bincount(np.minimum(w.slot_tri, n_tris), minlength=n_tris + 1)
    w.slot_bad = (w.slot_tri >= n_tris) | (seen[np.minimum(w.slot_tri, n_tris)] > 1)
    # ok, bottom-up: no defect of the shape below this child
    w.ok = np.ones(n, bool)
    w.ok[w.bad_run | w.overlap | (w.leaf & (w.count == 0))] = False
    w.ok[~w.leaf & (w.child0 < 0)] = False  # an inner reference the walk did not follow (out of range, or reached before)
    leaf_of_slot = np.full(n_tris, -1, np.int64)
    le = np.nonzero(w.leaf & (w.count > 0))[0]
    leaf_of_slot[_ranges(w.first[le], w.count[le])] = np.repeat(le, w.count[le])
    hit = leaf_of_slot[np.nonzero(w.slot_bad)[0]]
    w.ok[hit[hit >= 0]] = False
    w.size = w.count.copy()
    for lv in range(w.depth, 0, -1):
        e = np.nonzero(w.level == lv)[0]
        np.add.at(w.size, w.parent[e], w.size[e])
        np.logical_and.at(w.ok, w.parent[e], w.ok[e])
    # offsets, top-down: side 0 starts where the node starts, side 1 behind side 0
    w.off = np.zeros(n, np.int64)
    for lv in range(0, w.depth + 1):
        e = np.nonzero(w.level == lv)[0]
        start = np.where(w.parent[e] >= 0, w.off[np.maximum(w.parent[e], 0)], 0)
        w.off[e] = start + np.where(w.side[e] == 1, w.size[np.maximum(e - 1, 0)], 0)
    w.total = int(w.size[w.parent < 0].sum())
    w.order = np.zeros(w.total, np.int64)
    w.order[_ranges(w.off[le], w.count[le])] = _ranges(w.first[le], w.count[le])
    return w


def _ranges(start, size):
    """concatenate(arange(start[i], start[i] + size[i]))"""
    if len(start) == 0:
        return np.zeros(0, np.int64)
    total = int(size.sum())
    begin = np.cumsum(size) - size
    return np.repeat(start - begin, size) + np.arange(total)


def _slot_vertices(arr, w):
    """(slots, 3, 3) float64: the three vertices of every slot's triangle (an index reported by check_shape reads triangle 0)."""
    tri = np.where(w.slot_bad, 0, w.slot_tri)
    return arr["verts"].astype(np.float64)[arr["tris"].astype(np.int64)[tri]]


# ------------------------------------------------------------------------------------------------------------------ shape
def check_shape(arr, w):
    n_tris = int(arr["nTris"])
    out = {"refs": list(w.bad_ref), "twice": list(w.twice)}
    pad = arr["bvh"]["pad"]
    bad = np.nonzero(w.visited & (pad != 0).any(1))[0]
    out["pad"] = [(int(i), int(pad[i, 0]), int(pad[i, 1])) for i in bad]
    runs = [(int(w.node[i]), int(w.side[i]), "count", int(w.ref[i])) for i in np.nonzero(w.bad_run)[0]]
    runs += [(int(w.node[i]), int(w.side[i]), "overlaps", int(w.first[i]), int(w.count[i])) for i in np.nonzero(w.overlap & ~w.bad_run)[0]]
    if not out["refs"] and not out["twice"]:  # (a walk that lost a subtree has said so: what it no longer covers is not a second finding)
        runs += [(int(s), "uncovered") for s in np.nonzero(w.cover == 0)[0]]
    out["leaf_runs"] = runs
    out["slot_perm"] = [(int(s), int(w.slot_tri[s])) for s in np.nonzero(w.slot_bad)[0]]
    if not w.slot_bad.any() and len(w.slot_tri) == n_tris:
        assert np.array_equal(np.sort(w.slot_tri), np.arange(n_tris))
    out["depth"] = [(int(w.depth),)] if w.depth > POINT_STACK_DEPTH else []
    out["deferred"] = [(int(w.node[i]), int(w.defer[i])) for i in np.nonzero(w.defer >= WAVE_STACK)[0][:16]]
    return out


# ------------------------------------------------------------------------------------------------------------------ boxes
def _by_side(w, a, b):
    """Per entry: its node's record for side 0 (a) or side 1 (b), widened."""
    return np.where((w.side == 0)[:, None], a[w.node], b[w.node]).astype(np.float64)


def check_boxes(arr, w, exact=True):
    """Every child box contains every vertex of the child's triangles (float32 widened exactly, no tolerance); exact: it IS their
    min / max bit for bit -- what pure min / max kernels and the host's median-split build give."""
    x = _slot_vertices(arr, w)[w.order]
    slo, shi = x.min(1), x.max(1)
    lo, hi = np.full((w.n, 3), np.inf), np.full((w.n, 3), -np.inf)
    le = np.nonzero(w.leaf & (w.count > 0))[0]
    if len(le):
        lo[le], hi[le] = _seg_reduce(np.minimum, slo, w.off[le], w.count[le]), _seg_reduce(np.maximum, shi, w.off[le], w.count[le])
    for lv in range(w.depth, 0, -1):
        e = np.nonzero(w.level == lv)[0]
        np.minimum.at(lo, w.parent[e], lo[e])
        np.maximum.at(hi, w.parent[e], hi[e])
    bvh = arr["bvh"]
    blo, bhi = _by_side(w, bvh["lo0"], bvh["lo1"]), _by_side(w, bvh["hi0"], bvh["hi1"])
    outside = ~((blo <= lo) & (bhi >= hi)).all(1)  # (written so that a NaN offends)
    unequal = ~((blo == lo) & (bhi == hi)).all(1) if exact else np.zeros(w.n, bool)
    bad = np.nonzero(w.ok & (outside | unequal))[0]
    return [(int(w.node[i]), int(w.side[i]), "does not contain" if outside[i] else "is not the min / max", blo[i].tolist(), bhi[i].tolist(),
             lo[i].tolist(), hi[i].tolist()) for i in bad]


# ------------------------------------------------------------------------------------------------------------------ slabs
def _slab_fields(arr, w):
    s = arr["slabs"]
    g, n = _by_side(w, s["g0"], s["g1"]), _by_side(w, s["n0"], s["n1"])
    return g[:, :3], g[:, 3], n[:, :3], n[:, 3]


def check_slabs(arr, w, max_slab_tris=SLAB_MAX_TRIS):
    """NodeSlab of every reachable child: form (rho finite and positive; n exactly zero or unit to 1e-6 in |n|^2; "no slab" only as
    e == -1, n == 0 on children of more than max_slab_tris triangles), and containment in float64 with zero tolerance: every vertex v of
    the child's triangles has |v - g| <= rho and, when e >= 0, |n . (v - g)| <= e."""
    g, rho, n, e = _slab_fields(arr, w)
    n2 = (n * n).sum(1)
    form = ~(np.isfinite(rho) & (rho > 0))
    form |= ~(((n == 0).all(1)) | (np.abs(n2 - 1.0) <= FRAME_TOL))
    form |= ~np.isfinite(g).all(1)
    none = ~(e >= 0)
    form |= none & ~((e == -1.0) & (n == 0).all(1) & (w.size > max_slab_tris))
    out = {"slab_form": [(int(w.node[i]), int(w.side[i]), float(rho[i]), n[i].tolist(), float(e[i]), int(w.size[i])) for i in np.nonzero(w.ok & form)[0]],
           "slab_rho": [], "slab_e": []}
    x = _slot_vertices(arr, w)[w.order]
    for lv in range(w.depth + 1):
        en = np.nonzero((w.level == lv) & w.ok & (w.size > 0))[0]
        if not len(en):
            continue
        rows = _ranges(w.off[en], w.size[en])
        d = x[rows] - np.repeat(g[en], w.size[en], axis=0)[:, None, :]
        r = np.sqrt((d * d).sum(2)).max(1)
        t = np.abs((d * np.repeat(n[en], w.size[en], axis=0)[:, None, :]).sum(2)).max(1)
        begin = np.cumsum(w.size[en]) - w.size[en]
        r, t = _seg_reduce(np.maximum, r, begin, w.size[en]), _seg_reduce(np.maximum, t, begin, w.size[en])
        for i in np.nonzero(~(r <= rho[en]))[0]:
            out["slab_rho"].append((int(w.node[en[i]]), int(w.side[en[i]]), float(r[i]), float(rho[en[i]])))
        for i in np.nonzero((e[en] >= 0) & ~(t <= e[en]))[0]:
            out["slab_e"].append((int(w.node[en[i]]), int(w.side[en[i]]), float(t[i]), float(e[en[i]])))
    return out


# ------------------------------------------------------------------------------------------------------------------ triangle records
def _records(arr):
    p = arr["triPre"].astype(np.float64)
    return p[:, 0:3], p[:, 3], p[:, 4:7], p[:, 7], p[:, 8:11]  # g, hu, n, hv, u


def check_records(arr, w):
    """triPre per slot: framed (n, u orthonormal to 1e-6; the vertices within 4e-7 of the scale of the plane, within hu along u and
    within hv across it, the last two with no tolerance) or a ball (n == u == 0, hu == 0, the vertices within hv of g)."""
    g, hu, n, hv, u = _records(arr)
    x = _slot_vertices(arr, w)
    scale = mesh_scale(arr["verts"])
    ball = (n == 0).all(1) & (u == 0).all(1)
    use = ~w.slot_bad
    d = x - g[:, None, :]
    r2 = (d * d).sum(2)
    s, a = (d * n[:, None, :]).sum(2), (d * u[:, None, :]).sum(2)
    frame = ~((np.abs((n * n).sum(1) - 1.0) <= FRAME_TOL) & (np.abs((u * u).sum(1) - 1.0) <= FRAME_TOL) & (np.abs((n * u).sum(1)) <= FRAME_TOL))
    plane = ~(np.abs(s).max(1) <= 4e-7 * scale)
    along = ~(np.abs(a).max(1) <= hu)
    across = ~(np.sqrt(np.maximum(r2 - s * s - a * a, 0.0)).max(1) <= hv)
    round_ = ~((hu == 0) & (np.sqrt(r2).max(1) <= hv))

    def rows(mask, *vals):
        return [(int(i),) + tuple(np.asarray(v[i]).tolist() for v in vals) for i in np.nonzero(mask)[0]]
    return {"record_frame": rows(use & ~ball & frame, n, u),
            "record_plane": rows(use & ~ball & ~frame & plane, np.abs(s).max(1)),
            "record_hu": rows(use & ~ball & along, np.abs(a).max(1), hu),
            "record_hv": rows(use & ~ball & across, hv),
            "record_ball": rows(use & ball & round_, hu, hv)}


# ------------------------------------------------------------------------------------------------------------------ triPos
def check_tripos(arr):
    """The nine coordinates are the bits of verts[tris]; the normal is cross(b - a, c - a) in float32, one operation per statement (the
    library is built with -ffp-contract=off)."""
    v, t, p = arr["verts"], arr["tris"].astype(np.int64), arr["triPos"]
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac = b - a, c - a
    m0, m1 = ab[:, [1, 2, 0]] * ac[:, [2, 0, 1]], ab[:, [2, 0, 1]] * ac[:, [1, 2, 0]]
    want = np.concatenate([a, b, c, m0 - m1], 1).astype(np.float32)
    bad = np.nonzero((want.view(np.uint32) != np.ascontiguousarray(p).view(np.uint32)).any(1))[0]
    return [(int(i), want[i].tolist(), p[i].tolist()) for i in bad]


# ------------------------------------------------------------------------------------------------------------------ twins
def _edges(tris):
    t = np.asarray(tris).astype(np.int64)
    return t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)  # half-edge c runs from tris.flat[c] to the triangle's next corner


def twins_manifold(tris):
    """Every directed edge once, its reverse once: a dictionary pairs them."""
    a, b = _edges(tris)
    where = dict(zip(((a << 32) | b).tolist(), range(len(a))))
    return np.array([where.get(k, 0xFFFFFFFF) for k in ((b << 32) | a).tolist()], np.uint32)


def twins_sequential(tris):
    """The reference's one pass in index order (Mesh::CreateHalfEdges): an edge whose reverse is in the map is paired with the reverse's
    FIRST owner (both entries are overwritten, the map keeps the owner); otherwise the edge is inserted unless its direction is there."""
    a, b = _edges(tris)
    he, owner = np.full(len(a), 0xFFFFFFFF, np.uint32), {}
    for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        j = owner.get((y, x))
        if j is not None:
            he[j], he[i] = i, j
        else:
            owner.setdefault((x, y), i)
    return he


def check_twins(arr, manifold=True):
    """he[c] is the edge at c reversed, everywhere.  Manifold: an involution without fixed points, equal to the dictionary pairing.
    Otherwise: equal to the sequential first-owner-wins pairing."""
    he = arr["halfEdges"].astype(np.int64)
    a, b = _edges(arr["tris"])
    inside = he < len(he)
    h = np.where(inside, he, 0)
    bad = ~inside | (a[h] != b) | (b[h] != a)
    if manifold:
        bad |= (h[h] != np.arange(len(he))) | (h == np.arange(len(he)))
        bad |= he != twins_manifold(arr["tris"])
    else:
        bad |= he != twins_sequential(arr["tris"])
    return [(int(c), int(he[c])) for c in np.nonzero(bad)[0]]


def check_structure(arr, exact_boxes=True, manifold=True, max_slab_tris=SLAB_MAX_TRIS):
    """Every structural check: name -> offenders."""
    w = walk(arr)
    out = check_shape(arr, w)
    out["boxes"] = check_boxes(arr, w, exact_boxes)
    if arr["slabs"] is not None:
        out.update(check_slabs(arr, w, max_slab_tris))
    out.update(check_records(arr, w))
    out["tripos"] = check_tripos(arr)
    out["twins"] = check_twins(arr, manifold)
    return out


# ------------------------------------------------------------------------------------------------------------------ the bounds as numbers
def tri_lower_bound2(p, g, hu, n, hv, u):
    """triLowerBound2's formula in float64 (broadcasting)."""
    d = p - g
    s, a = (d * n).sum(-1), (d * u).sum(-1)
    lat = np.sqrt(np.maximum((d * d).sum(-1) - s * s - a * a, 0.0))
    ou, ov = np.maximum(np.abs(a) - hu, 0.0), np.maximum(lat - hv, 0.0)
    return s * s + ou * ou + ov * ov


def slab_lower_bound2(p, g, rho, n, e):
    """slabLowerBound2's formula in float64 (broadcasting)."""
    d = p - g
    s = (d * n).sum(-1)
    al = np.maximum(np.abs(s) - e, 0.0)
    off = np.maximum(np.sqrt(np.maximum((d * d).sum(-1) - s * s, 0.0)) - rho, 0.0)
    return al * al + off * off


def _tri_distance(p, x):
    """Distance of points p (k, 3) from triangles x (k, 3, 3), row by row."""
    q = closest_point_on_triangle_f64(p, x[:, 0], x[:, 1], x[:, 2])
    return np.sqrt(((q - p) ** 2).sum(1))


def check_bounds(arr, w, pts, exhaustive):
    """sqrt(LB) <= d_true (1 + 1e-6) + 0.5 slack for the lower bounds the traversals prune by: triLowerBound2 on every record against
    its triangle, slabLowerBound2 on every child that has a slab against the nearest triangle of its run; d_true by
    helpers.closest_point_on_triangle_f64.
    The absolute share: of the slack, a quarter is closestSimplex's face-case tolerance and ~0.09 the rounding of its q (3 u M), which
    leaves ~0.66 for whatever a bound is off by; the test grants 0.5 and leaves the rest to the float32 evaluation of the bound on the
    device.
    The relative share: a frame stored in float32 is orthonormal to rounding, not exactly -- the records' own invariant is 1e-6 in
    |n|^2, |u|^2 and n . u (FRAME_TOL, check_records), the slabs' 1e-6 in |n|^2 -- so s^2 + a^2 may exceed the squared projection by
    (1 + 2e-6) and a distance formed from it the true one by 1e-6 OF ITSELF, in exact arithmetic.  The code's budget puts this where it
    puts every error that grows with the distance (meshSlack's comment: "|n| - 1: ~16 u D (factor)"): into rejectBound's factor
    1.00001, 5e-6 of the distance.  Without this term the comparison fails on points ~20 extents away from the flattened icosphere,
    where |n|^2 - 1 = 1.7e-7 of a record times d_true = 21.9 is 0.77 of the slack (8e-8 of the distance, a sixtieth of the factor).
    exhaustive: all points x all slots and all children; otherwise, per point, both children of every node on the path from the root
    towards the point's nearer box, and the records of the leaves met.
    Returns (offenders, worst): worst["records"], worst["slabs"] = the largest (sqrt(LB) - d_true) / slack seen, and
    worst["records_net"], worst["slabs_net"] the same with the relative share taken off, which is what is compared with 0.5."""
    slack = mesh_slack(arr["verts"])
    tol = BOUND_SHARE_OF_SLACK * slack
    g, hu, n, hv, u = _records(arr)
    x = _slot_vertices(arr, w)
    pts = np.asarray(pts, np.float64)
    have_slabs = arr["slabs"] is not None
    if have_slabs:
        sg, srho, sn, se = _slab_fields(arr, w)
    n_slots = len(x)
    use_slot = ~w.slot_bad
    offenders, worst = [], {"records": -np.inf, "slabs": -np.inf, "records_net": -np.inf, "slabs_net": -np.inf}

    def note(kind, lb, dist, describe):
        if lb.size:
            net = lb - dist * (1.0 + FRAME_TOL)
            worst[kind] = max(worst[kind], float(np.max(lb - dist)) / slack)
            worst[kind + "_net"] = max(worst[kind + "_net"], float(np.max(net)) / slack)
            for i in np.argwhere(net > tol)[:8]:
                offenders.append(describe(tuple(int(v) for v in i)) + (float(net[tuple(i)]) / slack, float(dist[tuple(i)])))

    if exhaustive:
        en = np.nonzero(w.ok & (w.size > 0) & (se >= 0))[0] if have_slabs else np.zeros(0, np.int64)
        levels = [en[w.level[en] == lv] for lv in range(w.depth + 1)]
        levels = [e for e in levels if len(e)]
        step = max(1, _CHUNK_ROWS // max(n_slots, 1))

        def chunk(k0):
            p = pts[k0:k0 + step]
            k = len(p)
            dist = _tri_distance(np.repeat(p, n_slots, axis=0), np.tile(x, (k, 1, 1))).reshape(k, n_slots)
            lb = np.sqrt(tri_lower_bound2(p[:, None, :], g[None], hu[None], n[None], hv[None], u[None]))
            res = [("records", np.where(use_slot[None, :], lb, -np.inf), dist, None)]
            dt = dist[:, w.order].T  # (traversal position, point)
            for e in levels:
                near = _seg_reduce(np.minimum, dt, w.off[e], w.size[e]).T
                sl = np.sqrt(slab_lower_bound2(p[:, None, :], sg[e][None], srho[e][None], sn[e][None], se[e][None]))
                res.append(("slabs", sl, near, e))
            return k0, res

        with ThreadPoolExecutor(_THREADS) as pool:
            for k0, res in pool.map(chunk, range(0, len(pts), step)):
                for kind, lb, dist, e in res:
                    if kind == "records":
                        note(kind, lb, dist, lambda i: ("record", k0 + i[0], i[1]))
                    else:
                        note(kind, lb, dist, lambda i: ("slab", k0 + i[0], int(w.node[e[i[1]]]), int(w.side[e[i[1]]])))
        return offenders, worst

    xo = x[w.order]
    cen = xo.mean(1)
    rad = np.sqrt(((xo - cen[:, None, :]) ** 2).sum(2)).max(1)
    bvh = arr["bvh"]
    blo, bhi = _by_side(w, bvh["lo0"], bvh["lo1"]), _by_side(w, bvh["hi0"], bvh["hi1"])

    def one(k):
        p = pts[k]
        lower = np.maximum(np.sqrt(((cen - p) ** 2).sum(1)) - rad, 0.0)  # <= the distance of every point of the triangle
        upper = np.sqrt(((xo[:, 0] - p) ** 2).sum(1))                  # >= it: the distance of a vertex
        slab_of, slab_pos, leaf_pos, e0 = [], [], [], 0
        while e0 >= 0:
            nxt, best = -1, np.inf
            for e in (e0, e0 + 1):
                if not (w.ok[e] and w.size[e] > 0):
                    continue
                o, sz = int(w.off[e]), int(w.size[e])
                if have_slabs and se[e] >= 0:
                    slab_of.append(e)
                    slab_pos.append(o + np.nonzero(lower[o:o + sz] <= upper[o:o + sz].min())[0])  # the run's nearest triangle is among these
                if w.leaf[e]:
                    leaf_pos.append(np.arange(o, o + sz))
                else:
                    far = np.sqrt((np.maximum(np.maximum(blo[e] - p, p - bhi[e]), 0.0) ** 2).sum())
                    if far < best:
                        best, nxt = far, int(w.child0[e])
            e0 = nxt
        # every exact distance of this point in one call
        pos = np.concatenate(slab_pos + leaf_pos)
        dist = _tri_distance(np.repeat(p[None], len(pos), 0), xo[pos])
        found = []
        if slab_of:
            size = np.array([len(c) for c in slab_pos])
            near = _seg_reduce(np.minimum, dist, np.cumsum(size) - size, size)
            en = np.array(slab_of)
            lb = np.sqrt(slab_lower_bound2(p[None], sg[en], srho[en], sn[en], se[en]))
            found.append(("slabs", lb, near, [(int(w.node[e]), int(w.side[e])) for e in en]))
        if leaf_pos:
            at = np.concatenate(leaf_pos)
            s, d = w.order[at], dist[len(pos) - len(at):]
            lb = np.sqrt(tri_lower_bound2(p[None], g[s], hu[s], n[s], hv[s], u[s]))
            found.append(("records", np.where(use_slot[s], lb, -np.inf), d, [(int(t),) for t in s]))
        return k, found

    with ThreadPoolExecutor(_THREADS) as pool:
        for k, found in pool.map(one, range(len(pts))):
            for kind, lb, dist, what in found:
                note(kind, lb, dist, lambda i: (kind, k) + what[i[0]])
    return offenders, worst
