"""The data the mesh traversals prune by, as the device build writes it (mesh_build.hip, mesh_tripre_kernel), downloaded once per
field through Field.mesh_arrays and checked on the host in float64 by tests/mesh_structure.py: child boxes, slabs, triangle records,
leaf runs and the slot -> triangle map, twins -- and the bounds as numbers against exact distances.  The end-to-end tests elsewhere
(hierarchy == scan == oracle) see a bound that is too tight only if a probe point sits where it prunes the winner; these see it in
the structure.  tests/test_mesh_structure_cpu.py shows that each check fails on a subtly wrong array."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_structure as MS
from conftest import bits
from helpers import displaced_torus, fuzz_mesh_case, hard_points, icosphere
from test_gpu_configs import _hard_meshes, _membrane_bipyramid

pytestmark = pytest.mark.gpu
EXHAUSTIVE_TRIS = 5200  # all points x all slots and children up to here; beyond, 256 points along their paths


def _tetrahedron():
    return (np.float32([[0.3, 0.3, 0.3], [-0.3, -0.3, 0.3], [-0.3, 0.3, -0.3], [0.3, -0.3, -0.3]]),
            np.uint64([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]))


def _octahedron():
    return (np.float32([[0.3, 0, 0], [-0.3, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.2], [0, 0, -0.2]]),
            np.uint64([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))


@functools.lru_cache(None)
def _hard_list():
    return [mesh for _, mesh in _hard_meshes()]


def _hard(k):
    return lambda: _hard_list()[k]


MESHES = {
    "tetrahedron": _tetrahedron,
    "octahedron": _octahedron,
    "icosphere 3": lambda: icosphere(3),
    "torus 48 x 32": lambda: displaced_torus(48, 32),
    "hard: icosphere 5": _hard(0),
    "hard: displaced torus": _hard(1),
    "hard: far from the origin": _hard(2),
    "hard: flattened": _hard(3),
    "hard: slivers": _hard(4),
    "needles 100758": lambda: fuzz_mesh_case(100758)[:2],
    "needles 910968": lambda: fuzz_mesh_case(910968)[:2],
    "membrane bipyramid": _membrane_bipyramid,
    "torus 512 x 320": lambda: displaced_torus(512, 320),
}
_cache = {}


def _mesh(name):
    if name not in _cache:
        _cache[name] = MESHES[name]()
    return _cache[name]


def _export(H, ctx, verts, tris):
    f = H.Field.mesh(ctx, verts, tris)
    try:
        return f.mesh_arrays(ctx)
    finally:
        f.close()


def _check(name, arr, verts, tris, leaf_tris, slabs=True, manifold=True, seed=0):
    """Every structural check, then the bounds as numbers; prints the worst (sqrt(LB) - d_true) / slack of the mesh.
    On an MI355X: as defined, up to 0.95 for records (3072-triangle torus, leaves of 1) and 0.77 (flattened icosphere), all of it on
    hard_points' probes 10 extents and more away and all of it the float32 rounding of the stored unit vectors times the distance
    (mesh_structure.check_bounds has the account); with that relative share (1e-6 of d_true) taken off, at most 0.021 for records
    (the mesh far from the origin) and 0.000 for slabs on every mesh here, against the predicted ~0.2 and the cap of 0.5."""
    assert H_DTYPES["bvh"] == MS.BVH_DTYPE and H_DTYPES["slabs"] == MS.SLAB_DTYPE
    assert arr["nVerts"] == len(verts) and arr["nTris"] == len(tris) and 1 << arr["leafLog2"] >= leaf_tris > (1 << arr["leafLog2"]) // 2
    assert np.array_equal(arr["verts"].view(np.uint32), np.ascontiguousarray(verts, np.float32).view(np.uint32))
    assert np.array_equal(arr["tris"], tris.astype(np.uint32))
    assert (arr["slabs"] is not None) == slabs
    res = MS.check_structure(arr, exact_boxes=True, manifold=manifold)
    for check, offenders in res.items():
        assert not offenders, "%s, %s: %s" % (name, check, MS.first(offenders))
    w = MS.walk(arr)
    assert w.total == len(tris) and w.ok.all()
    pts = hard_points(verts, tris.astype(np.int64), seed)
    exhaustive = len(tris) <= EXHAUSTIVE_TRIS
    if not exhaustive:
        pts = pts[np.linspace(0, len(pts) - 1, 256).astype(np.int64)]  # (every kind of point hard_points makes)
    offenders, worst = MS.check_bounds(arr, w, pts, exhaustive)
    print("%s (%d triangles, leaves of %d%s): worst (sqrt(LB) - d_true) / slack: records %.4f, slabs %.4f; less 1e-6 d_true: records %.4f, "
          "slabs %.4f (predicted ~0.2, cap %.1f)" % (name, len(tris), leaf_tris, "" if slabs else ", no slabs", worst["records"], worst["slabs"],
                                                    worst["records_net"], worst["slabs_net"], MS.BOUND_SHARE_OF_SLACK))
    assert not offenders, "%s: %s" % (name, MS.first(offenders))
    return w


H_DTYPES = {}


@pytest.fixture(autouse=True)
def _dtypes(H):
    H_DTYPES.update(bvh=H.BVH_DTYPE, slabs=H.SLAB_DTYPE)


@pytest.mark.parametrize("name", [n for n in MESHES if n not in ("torus 512 x 320", "membrane bipyramid")])
def test_device_built_structure(H, ctx, name):
    verts, tris = _mesh(name)
    w = _check(name, _export(H, ctx, verts, tris), verts, tris, 8, seed=len(tris))
    if len(tris) <= 8:
        assert w.n == 2 and w.leaf.all()  # the root's children are leaves


def test_non_manifold_twins_come_from_the_host_everything_else_from_the_device(H, ctx):
    verts, tris = _mesh("membrane bipyramid")
    assert len(MS.check_twins(dict(tris=tris, halfEdges=MS.twins_sequential(tris)), manifold=True)) > 0  # (no involution here)
    _check("membrane bipyramid", _export(H, ctx, verts, tris), verts, tris, 8, manifold=False, seed=5)


@pytest.mark.parametrize("leaf_tris", [1, 8, 16])
@pytest.mark.parametrize("name", ["torus 48 x 32", "torus 512 x 320"])
def test_leaf_sizes_and_the_three_slab_regimes(H, ctx, monkeypatch, name, leaf_tris):
    """3072 triangles: children above and below the 1024 that send a child to the workgroup kernel.  327 680 triangles: the root's
    children (~164 k, more than 131 072) have no slab, their descendants above 1024 triangles take the workgroup kernel's list, the
    rest a wave each; 1280 workgroups fit the boxes, so hand-overs cross XCDs."""
    monkeypatch.setenv("HPSDF_MESH_LEAF_TRIS", str(leaf_tris))
    verts, tris = _mesh(name)
    arr = _export(H, ctx, verts, tris)
    w = _check(name, arr, verts, tris, leaf_tris, seed=leaf_tris)
    _, _, _, e = MS._slab_fields(arr, w)
    big = w.size > MS.SLAB_MAX_TRIS
    assert np.array_equal(e < 0, big) and big.any() == (len(tris) > 2 * MS.SLAB_MAX_TRIS)
    assert ((w.size > 1024) & ~big).any() and (w.size <= 1024).any()


@pytest.mark.parametrize("name", ["torus 48 x 32", "hard: slivers"])
def test_boxes_only_and_host_built_fields(H, ctx, monkeypatch, name):
    verts, tris = _mesh(name)
    monkeypatch.setenv("HPSDF_MESH_NO_SLABS", "1")
    _check(name, _export(H, ctx, verts, tris), verts, tris, 8, slabs=False, seed=1)
    monkeypatch.delenv("HPSDF_MESH_NO_SLABS")
    monkeypatch.setenv("HPSDF_MESH_HOST_BUILD", "1")
    arr = _export(H, ctx, verts, tris)
    w = _check(name + ", host build", arr, verts, tris, 1, slabs=False, seed=2)  # (median split, exact min / max boxes: mesh.cpp)
    assert w.leaf.sum() == len(tris) and np.array_equal(w.slot_tri, np.arange(len(tris))) and w.depth <= 31


def test_the_build_is_deterministic(H, ctx):
    """Two fields from the large mesh: the same bytes.  (Slabs: of the nodes a traversal can reach -- mb_slab_kernel leaves the
    records of nodes below a leaf unwritten, and nothing refers to them.)"""
    verts, tris = _mesh("torus 512 x 320")
    a, b = _export(H, ctx, verts, tris), _export(H, ctx, verts, tris)
    for k in ("bvh", "triPre", "halfEdges", "triPos"):
        assert a[k].tobytes() == b[k].tobytes(), k
    reached = MS.walk(a).visited
    assert reached.sum() > 30000 and a["slabs"][reached].tobytes() == b["slabs"][reached].tobytes()


def test_the_exports_contract(H, ctx):
    verts, tris = _mesh("icosphere 3")
    f = H.Field.mesh(ctx, verts, tris)
    call = H.lib().hpsdf_field_mesh_arrays
    info = (C.c_uint64 * 5)(*[77] * 5)
    assert call(f.handle, info, None, None) == H.OK and list(info) == [len(verts), len(tris), len(tris) - 1, 3, 1]
    arr = f.mesh_arrays(ctx)
    need = [arr[k].nbytes for k in ("verts", "tris", "triPos", "triPre", "halfEdges", "bvh", "slabs")]
    assert need == [12 * len(verts), 12 * len(tris), 48 * len(tris), 48 * len(tris), 12 * len(tris), 64 * (len(tris) - 1), 64 * (len(tris) - 1)]
    # one buffer a byte short: refused, and nothing is written -- neither the buffers nor info
    for short in range(7):
        bufs = [np.full(n, 0xAB, np.uint8) for n in need]
        caps = (C.c_uint64 * 7)(*[n - (i == short) for i, n in enumerate(need)])
        info = (C.c_uint64 * 5)(*[77] * 5)
        assert call(f.handle, info, (C.c_void_p * 7)(*[b.ctypes.data for b in bufs]), caps) == H.ERR_INVALID_ARGUMENT
        assert list(info) == [77] * 5 and all((b == 0xAB).all() for b in bufs)
    assert call(f.handle, info, (C.c_void_p * 7)(*[b.ctypes.data for b in bufs]), None) == H.ERR_INVALID_ARGUMENT
    # a null entry is skipped; capacities may exceed the need
    bvh = np.full(need[5] + 64, 0xAB, np.uint8)
    ptrs = (C.c_void_p * 7)(None, None, None, None, None, bvh.ctypes.data, None)
    assert call(f.handle, info, ptrs, (C.c_uint64 * 7)(*[0, 0, 0, 0, 0, len(bvh), 0])) == H.OK
    assert bvh[:need[5]].tobytes() == arr["bvh"].tobytes() and (bvh[need[5]:] == 0xAB).all()
    f.close()
    # fields that are not meshes are refused
    for g in (H.Field.sphere(), H.Field.callback(lambda p, t: 0.0)):
        info = (C.c_uint64 * 5)(*[77] * 5)
        assert call(g.handle, info, None, None) == H.ERR_INVALID_ARGUMENT and list(info) == [77] * 5
        with pytest.raises(H.HpsdfError) as e:
            g.mesh_arrays(ctx)
        assert e.value.status == H.ERR_INVALID_ARGUMENT
        g.close()
    assert call(None, info, None, None) == H.ERR_INVALID_ARGUMENT


def test_the_export_leaves_the_field_and_its_host_copies_alone(H, ctx):
    """Calls of one point are answered from the field's host mirror, which the same download fills: the same bits before the export,
    after it, after the mirror has been dropped and fetched again -- and the bits of the device's scan."""
    verts, tris = _mesh("torus 48 x 32")
    f = H.Field.mesh(ctx, verts, tris)
    pts = hard_points(verts, tris.astype(np.int64), 9)[::200]
    first = f.mesh_arrays(ctx)
    before = np.array([f.eval(ctx, p[None])[0] for p in pts])
    again = f.mesh_arrays(ctx)
    after = np.array([f.eval(ctx, p[None])[0] for p in pts])
    f.release_host_copies()
    fresh = np.array([f.eval(ctx, p[None])[0] for p in pts])
    assert np.array_equal(bits(before), bits(after)) and np.array_equal(bits(before), bits(fresh))
    assert np.array_equal(bits(before), bits(f.eval_naive(ctx, pts)))
    for k in ("verts", "tris", "triPos", "triPre", "halfEdges", "bvh"):
        assert first[k].tobytes() == again[k].tobytes() == f.mesh_arrays(ctx)[k].tobytes(), k
    f.close()
