"""The mesh-structure checker (tests/mesh_structure.py) on a hierarchy built here in numpy, without a device: it accepts a valid one,
and each single defect a kernel could produce is reported by the check that owns it and by no other -- which is what makes
tests/test_gpu_mesh_structure.py a test of the device build rather than of its own leniency."""
import numpy as np
import pytest

import mesh_structure as MS
from helpers import hard_points, icosphere

LEAF_TRIS = 8


def _up(x):
    """float64 -> the float32 at or above it, and one more (the checker's own float64 evaluation may round the other way)."""
    f = np.asarray(x, np.float64).astype(np.float32)
    f = np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)
    return np.nextafter(f, np.float32(np.inf))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def build_hierarchy(verts, tris, leaf_tris=LEAF_TRIS):
    """A valid hierarchy in the exported layout: median split on the longest axis of the centroids, leaves of <= leaf_tris triangles
    in slot order, exact boxes, slabs and triangle records computed in float64 against the float32 values that are stored and
    rounded outward."""
    v32, t = np.asarray(verts, np.float32), np.asarray(tris).astype(np.int64)
    n_tris = len(t)
    x = v32.astype(np.float64)[t]
    cen = x.mean(1)
    nodes, slot_tri = [], []

    def split(ids):
        if len(ids) <= leaf_tris:
            first = len(slot_tri)
            slot_tri.extend(ids.tolist())
            return ~((first << MS.LEAF_SHIFT) | (len(ids) - 1)), ids
        axis = int(np.argmax(cen[ids].max(0) - cen[ids].min(0)))
        ids = ids[np.argsort(cen[ids, axis], kind="stable")]
        me = len(nodes)
        nodes.append(None)
        nodes[me] = split(ids[:len(ids) // 2]) + split(ids[len(ids) // 2:])
        return me, ids

    assert split(np.arange(n_tris))[0] == 0
    bvh, slabs = np.zeros(len(nodes), MS.BVH_DTYPE), np.zeros(len(nodes), MS.SLAB_DTYPE)
    area_normal = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    for k, (c0, ids0, c1, ids1) in enumerate(nodes):
        bvh["c0"][k], bvh["c1"][k] = c0, c1
        for side, ids in ((0, ids0), (1, ids1)):
            pts = x[ids].reshape(-1, 3)
            lo, hi = pts.min(0), pts.max(0)
            bvh["lo%d" % side][k], bvh["hi%d" % side][k] = lo, hi
            n = _unit(area_normal[ids].sum(0)).astype(np.float32).astype(np.float64)
            c = 0.5 * (lo + hi)
            along = (pts - c) @ n
            g = (c + 0.5 * (along.min() + along.max()) * n).astype(np.float32).astype(np.float64)
            d = x[ids] - g
            slabs["g%d" % side][k] = np.concatenate([g, _up(np.sqrt((d * d).sum(2)).max())[None]])
            slabs["n%d" % side][k] = np.concatenate([n, _up(np.abs((d * n).sum(2)).max())[None]])
    # triangle records, per slot
    xs = x[slot_tri]
    edges = np.stack([xs[:, 1] - xs[:, 0], xs[:, 2] - xs[:, 0], xs[:, 2] - xs[:, 1]], 1)
    longest = edges[np.arange(n_tris), np.argmax((edges ** 2).sum(2), 1)]
    n = _unit(np.cross(edges[:, 0], edges[:, 1])).astype(np.float32).astype(np.float64)
    u = _unit(longest).astype(np.float32).astype(np.float64)
    v = np.cross(n, u)
    pu, pv = ((xs - xs[:, :1]) * u[:, None]).sum(2), ((xs - xs[:, :1]) * v[:, None]).sum(2)
    g = xs[:, 0] + (0.5 * (pu.min(1) + pu.max(1)))[:, None] * u + (0.5 * (pv.min(1) + pv.max(1)))[:, None] * v
    g = g.astype(np.float32).astype(np.float64)
    d = xs - g[:, None]
    s, a = (d * n[:, None]).sum(2), (d * u[:, None]).sum(2)
    hu = _up(np.abs(a).max(1))
    hv = _up(np.sqrt(np.maximum((d * d).sum(2) - s * s - a * a, 0.0)).max(1))
    tri_pre = np.zeros((n_tris, 12), np.float32)
    tri_pre[:, 0:3], tri_pre[:, 3], tri_pre[:, 4:7], tri_pre[:, 7], tri_pre[:, 8:11] = g, hu, n, hv, u
    tri_pre[:, 11] = np.array(slot_tri, np.uint32).view(np.float32)
    # triPos in float32, one operation per statement
    a32, b32, c32 = v32[t[:, 0]], v32[t[:, 1]], v32[t[:, 2]]
    ab, ac = b32 - a32, c32 - a32
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    tri_pos = np.concatenate([a32, b32, c32, np.stack([nx, ny, nz], 1)], 1).astype(np.float32)
    # twins: sort the directed edges, look the reverse up
    src, dst = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    key, rev = src * len(v32) + dst, dst * len(v32) + src
    by_key = np.argsort(key)
    he = by_key[np.searchsorted(key[by_key], rev)].astype(np.uint32)
    leaf_log2 = int(np.ceil(np.log2(leaf_tris)))
    return dict(verts=v32, tris=t.astype(np.uint32), triPos=tri_pos, triPre=tri_pre, halfEdges=he, bvh=bvh, slabs=slabs,
                nVerts=len(v32), nTris=n_tris, nBvhNodes=len(nodes), leafLog2=leaf_log2)


@pytest.fixture(scope="module")
def valid():
    verts, tris = icosphere(2)
    return build_hierarchy(verts, tris)


def _copy(arr):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in arr.items()}


def _failing(arr, **kw):
    return sorted(k for k, v in MS.check_structure(arr, **kw).items() if v)


def test_the_checker_accepts_a_valid_hierarchy(valid):
    w = MS.walk(valid)
    assert w.total == valid["nTris"] == 320 and w.ok.all() and w.depth >= 5
    assert np.array_equal(np.sort(w.order), np.arange(320))
    res = MS.check_structure(valid)
    assert set(res) == {"refs", "twice", "pad", "leaf_runs", "slot_perm", "depth", "deferred", "boxes", "slab_form", "slab_rho", "slab_e",
                        "record_frame", "record_plane", "record_hu", "record_hv", "record_ball", "tripos", "twins"}
    for name, offenders in res.items():
        assert not offenders, name + ": " + MS.first(offenders)
    # without slabs (host-built fields, HPSDF_MESH_NO_SLABS) the rest holds
    bare = _copy(valid)
    bare["slabs"] = None
    assert _failing(bare) == []


def _leaf_entry(w, room=False):
    """A leaf deep in the tree (with room for one more triangle, and a run behind it)."""
    ok = w.leaf & (w.level == w.depth)
    if room:
        ok &= (w.count < (1 << w.leaf_log2)) & (w.first + w.count < len(w.slot_tri))
    return int(np.nonzero(ok)[0][0])


def _set_ref(arr, w, e, value):
    arr["bvh"]["c%d" % w.side[e]][w.node[e]] = value


def _box_face_inward(arr, w):
    e = _leaf_entry(w)
    lo = arr["bvh"]["lo%d" % w.side[e]]
    lo[w.node[e], 1] = np.nextafter(lo[w.node[e], 1], np.float32(np.inf))


def _slab_word(arr, w, field, factor):
    e = _leaf_entry(w)
    rec = arr["slabs"]["%s%d" % (field, w.side[e])]
    assert rec[w.node[e], 3] > 0
    rec[w.node[e], 3] *= np.float32(factor)


def _hu_reduced(arr, w):
    arr["triPre"][17, 3] *= np.float32(1 - 1e-4)


def _normal_scaled(arr, w):
    arr["triPre"][23, 4:7] *= np.float32(1.001)


def _equal_indices(arr, w):
    arr["triPre"][40, 11] = arr["triPre"][200, 11]


def _leaf_overlaps(arr, w):
    e = _leaf_entry(w, room=True)
    _set_ref(arr, w, e, int(w.ref[e]) - 1)  # ~c + 1: one more triangle, the first of the next run


def _pad_word(arr, w):
    arr["bvh"]["pad"][int(w.node[_leaf_entry(w)]), 1] = 0xFFFFFFFF


def _cycle(arr, w):
    e = int(np.nonzero(~w.leaf & (w.level == 3))[0][0])
    _set_ref(arr, w, e, int(w.node[w.parent[w.parent[e]]]))  # back to its grandparent


def _twin_redirected(arr, w):
    arr["halfEdges"][5] = arr["halfEdges"][11]


def _tripos_normal(arr, w):
    arr["triPos"][99, 10] = np.nextafter(arr["triPos"][99, 10], np.float32(np.inf))


MUTATIONS = {
    "one box face moved inward by one float32 ulp": (_box_face_inward, "boxes"),
    "one slab e reduced by 1e-4 of itself": (lambda a, w: _slab_word(a, w, "n", 1 - 1e-4), "slab_e"),
    "one rho reduced by 1e-4 of itself": (lambda a, w: _slab_word(a, w, "g", 1 - 1e-4), "slab_rho"),
    "one record's hu reduced by 1e-4 of itself": (_hu_reduced, "record_hu"),
    "one record's n scaled by 1.001": (_normal_scaled, "record_frame"),
    "two slots with the same triangle index": (_equal_indices, "slot_perm"),
    "a leaf count that overlaps the next run": (_leaf_overlaps, "leaf_runs"),
    "a non-zero pad word": (_pad_word, "pad"),
    "a child reference that makes a cycle": (_cycle, "twice"),
    "one twin redirected": (_twin_redirected, "twins"),
    "one triPos normal off by an ulp": (_tripos_normal, "tripos"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_each_defect_is_reported_by_its_own_check_alone(valid, what):
    mutate, owner = MUTATIONS[what]
    arr = _copy(valid)
    mutate(arr, MS.walk(valid))
    assert _failing(arr) == [owner]


def test_further_defects_of_the_shape(valid):
    w = MS.walk(valid)
    arr = _copy(valid)
    _set_ref(arr, w, _leaf_entry(w), valid["nBvhNodes"] + 3)
    assert _failing(arr) == ["refs"]
    arr = _copy(valid)
    arr["leafLog2"] = 2  # leaves of five triangles under a field that promises four
    assert _failing(arr) == ["leaf_runs"]
    arr = _copy(valid)
    e = _leaf_entry(w)
    arr["slabs"]["n%d" % w.side[e]][w.node[e]] = (0, 0, 0, -1)  # "no slab" on a child small enough to have one
    assert _failing(arr) == ["slab_form"]
    arr = _copy(valid)
    arr["triPre"][7, 4:11] = 0  # a ball that kept its hu
    assert _failing(arr) == ["record_ball"]
    arr["triPre"][7, 3] = 0
    assert _failing(arr) == ["record_ball"]  # ... and whose hv is the rectangle's, not a radius around g
    arr["triPre"][7, 7] = 0.1
    assert _failing(arr) == []
    # a chain deeper than the per-point stack: 97 inner nodes in a row, each with a leaf beside
    deep = np.zeros(98, MS.BVH_DTYPE)
    deep["c0"], deep["c1"] = ~np.int32(0), np.arange(1, 99)
    deep["c1"][97] = ~np.int32(0)
    chain = MS.walk(dict(bvh=deep, nTris=1, leafLog2=0, triPre=np.zeros((1, 12), np.float32)))
    assert chain.depth == 97 and MS.check_shape(dict(bvh=deep, nTris=1), chain)["depth"] == [(97,)]
    assert MS.check_shape(valid, w)["depth"] == [] and w.defer.max() < MS.WAVE_STACK


def test_twin_pairings():
    verts, tris = icosphere(1)
    he = MS.twins_manifold(tris)
    assert np.array_equal(he, MS.twins_sequential(tris)) and np.array_equal(he[he], np.arange(len(he)))
    # three faces on one edge, the direction that occurs once first: the first owner is paired twice, the LAST pairing stands
    fan = np.array([[1, 0, 2], [0, 1, 3], [0, 1, 4]])
    he = MS.twins_sequential(fan)
    assert he[0] == 6 and he[3] == 0 and he[6] == 0
    arr = dict(tris=fan.astype(np.uint32), halfEdges=he)
    bad = MS.check_twins(arr, manifold=False)
    assert all(c not in (0, 3, 6) for c, _ in bad)  # (the other edges of the fan are open)
    assert any(c == 3 for c, _ in MS.check_twins(arr, manifold=True))


def test_the_bounds_as_numbers(valid):
    """The valid hierarchy's bounds are exact up to the float32 rounding of what is stored: the frame's (a part in 1e7 of the distance:
    0.2 of the slack on the points 10 extents away, the relative share check_bounds takes off) and g's (0.01 of the slack), so nothing
    comes near the 0.5 the device is granted; a bound that is too tight by more than that is reported, by the exhaustive comparison
    and by the one along the points' paths."""
    pts = hard_points(valid["verts"], valid["tris"].astype(np.int64), 1)
    w = MS.walk(valid)
    for exhaustive in (True, False):
        offenders, worst = MS.check_bounds(valid, w, pts if exhaustive else pts[::8], exhaustive)
        assert not offenders, MS.first(offenders)
        assert worst["records_net"] <= 0.02 and worst["slabs_net"] <= 0.02 and worst["records"] <= 0.3, worst
    arr = _copy(valid)
    arr["triPre"][:, 3] *= np.float32(0.5)
    for exhaustive in (True, False):
        offenders, worst = MS.check_bounds(arr, w, pts[::8], exhaustive)
        assert offenders and all(o[0].startswith("record") for o in offenders) and worst["records_net"] > 0.5 >= worst["slabs_net"]
    arr = _copy(valid)
    arr["slabs"]["n0"][:, 3] = 0
    arr["slabs"]["n1"][:, 3] = 0
    for exhaustive in (True, False):
        offenders, worst = MS.check_bounds(arr, w, pts[::8], exhaustive)
        assert offenders and all(o[0].startswith("slab") for o in offenders) and worst["slabs_net"] > 0.5 >= worst["records_net"]
