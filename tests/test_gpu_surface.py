"""hpsdf_extract_surface on the device: lattice values bitwise equal to Query, the whole mesh bitwise equal to the numpy restatement
(tests/surface_reference.py), topology and geometry against the analytic fields, determinism, argument errors, the round trip
through the mesh ingest, and the C++ drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import surface_reference as S
from test_surface_cpu import build_surface_prog

pytestmark = pytest.mark.gpu

ROOT_LO, ROOT_HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.3
TORUS_C, TORUS_R, TORUS_T = (0.01, 0.02, -0.03), 0.25, 0.08
SPHERE_TARGET = 1e-6


@pytest.fixture(scope="module")
def trees(H, ctx):
    out = {}
    for name, field, target in (("union3_top", H.Field.union3(), 1e-5), ("union3_general", H.Field.union3(), 1e-7),
                                ("sphere", H.Field.sphere(SPHERE_C, SPHERE_R), SPHERE_TARGET),
                                ("torus", H.Field.analytic([(H.PRIM_TORUS_Y, H.OP_UNION, list(TORUS_C) + [TORUS_R, TORUS_T])]), 1e-6)):
        block, _ = H.create_block(ctx, H.make_config(target), field, 0)
        out[name] = H.DeviceTree(ctx, block)
    out["deep"] = H.DeviceTree(ctx, helpers.deep_chain_block(np.random.default_rng(5)))
    yield out
    for t in out.values():
        t.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


CASES = [
    ("union3_top", ROOT_LO, ROOT_HI, (48, 48, 48)),
    ("union3_general", ROOT_LO, ROOT_HI, (64, 64, 64)),
    ("union3_general", (-0.37, -0.41, -0.29), (0.23, 0.11, 0.31), (37, 64, 23)),  # off-centre, non-cubic
    ("union3_top", (-0.45, -0.3, -0.35), (0.4, 0.1, 0.05), (23, 41, 30)),
    ("deep", ROOT_LO, ROOT_HI, (40, 33, 47)),
    ("deep", (0.2, 0.21, 0.19), (0.5, 0.5, 0.5), (45, 37, 41)),  # the chain's corner: leaves down to depth 10
    ("sphere", ROOT_LO, ROOT_HI, (50, 50, 50)),
]


@pytest.mark.parametrize("name,lo,hi,n", CASES)
def test_lattice_values_are_query_and_mesh_is_the_restatement(H, trees, name, lo, hi, n):
    t = trees[name]
    iso = 0.0 if name != "deep" else float(np.median(t.query(S.lattice_points(lo, hi, n))))
    verts, tris, vals = t.extract_surface(lo, hi, n, iso, values=True)
    pts = S.lattice_points(lo, hi, n)
    want = t.query(pts)
    assert np.array_equal(bits(vals.ravel()), bits(want)), "lattice values differ from Query"
    rv, rt = S.extract(vals, lo, hi, n, iso, H.surface_case_table())
    assert len(rt) > 0
    assert verts.shape == rv.shape and tris.shape == rt.shape
    assert np.array_equal(bits(verts), bits(rv)), "vertex bits differ from the restatement"
    assert np.array_equal(tris, rt), "triangles differ from the restatement"


def near_surface_error(vals, n, iso):
    """delta: the largest |Query - exact SDF| at the ends of the crossing edges.  A vertex is the root of the chord of the tree's
    values at its edge's ends; those differ from the exact SDF by at most delta, and the exact SDF, convex along the edge, lies at
    most h^2 / (8 (r - h)) below its chord -- so |SDF(vertex) - iso| <= delta + h^2 / (8 (r - h)) (r: the level set's radius).  The
    ends of a crossing edge lie within h + delta of the level set (the SDF is 1-Lipschitz), so the lattice points within 2 h cover
    them.  delta is measured, not fitted; it is held below sqrt(target) -- the build's error is a sum of squared residuals."""
    h = 1.0 / n
    exact = np.linalg.norm(S.lattice_points(ROOT_LO, ROOT_HI, (n, n, n)) - np.array(SPHERE_C), axis=1) - SPHERE_R
    near = np.abs(exact - iso) <= 2 * h
    delta = float(np.abs(vals.ravel()[near] - exact[near]).max())
    assert delta <= np.sqrt(SPHERE_TARGET) and delta < h
    return delta


def test_sphere_topology_and_geometry(H, trees):
    n = 64
    t = trees["sphere"]
    verts, tris, vals = t.extract_surface(ROOT_LO, ROOT_HI, (n, n, n), values=True)
    assert S.unmatched_edges(tris) == [] and S.components(tris) == 1
    assert S.euler_characteristic(verts, tris) == 2
    h = 1.0 / n
    c = np.array(SPHERE_C)
    delta = near_surface_error(vals, n, 0.0)
    d = np.abs(np.linalg.norm(verts - c, axis=1) - SPHERE_R)
    assert d.max() <= delta + h * h / (8 * (SPHERE_R - h)) + 1e-12
    vol = S.signed_volume(verts, tris)
    bound = 4 * np.pi * (SPHERE_R + h) ** 2 * (delta + h * h / (8 * (SPHERE_R - h)) + 3 * h * h / (8 * (SPHERE_R - h)))
    assert vol > 0 and abs(vol - 4.0 / 3.0 * np.pi * SPHERE_R ** 3) <= bound


def test_torus_has_euler_characteristic_zero(trees):
    verts, tris = trees["torus"].extract_surface(ROOT_LO, ROOT_HI, (72, 72, 72))
    assert S.unmatched_edges(tris) == [] and S.components(tris) == 1
    assert S.euler_characteristic(verts, tris) == 0 and S.signed_volume(verts, tris) > 0


def test_union3_components_and_euler_characteristic(trees):
    """union3 (Field.union3): the sphere (r 0.18) reaches the torus's tube (0.166 from the sphere's centre to the tube's surface), and
    the box is apart from both (0.34 from the sphere's centre, the torus below y = -0.15 and the box above y = 0.10).  So: two
    components -- a solid torus with a bump (genus 1, chi 0) and a box (chi 2)."""
    verts, tris = trees["union3_general"].extract_surface(ROOT_LO, ROOT_HI, (128, 128, 128))
    assert S.unmatched_edges(tris) == []
    assert S.components(tris) == 2
    assert S.euler_characteristic(verts, tris) == 2


def test_iso_offsets_the_sphere_and_an_iso_above_everything_is_empty(H, ctx, trees):
    n = 48
    h = 1.0 / n
    t = trees["sphere"]
    verts, tris, vals = t.extract_surface(ROOT_LO, ROOT_HI, (n, n, n), iso=0.05, values=True)
    r = SPHERE_R + 0.05
    d = np.abs(np.linalg.norm(verts - np.array(SPHERE_C), axis=1) - r)
    assert S.unmatched_edges(tris) == [] and S.euler_characteristic(verts, tris) == 2
    assert d.max() <= near_surface_error(vals, n, 0.05) + h * h / (8 * (r - h)) + 1e-12
    L = H.lib()
    lo3, hi3 = (C.c_double * 3)(*ROOT_LO), (C.c_double * 3)(*ROOT_HI)
    n3 = (C.c_uint32 * 3)(16, 16, 16)
    v, tr = C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
    nv, nt = C.c_uint64(7), C.c_uint64(7)
    assert L.hpsdf_extract_surface(ctx.handle, t.handle, lo3, hi3, n3, 10.0, C.byref(v), C.byref(nv), C.byref(tr), C.byref(nt), None) == 0
    assert nv.value == 0 and nt.value == 0 and not v and not tr


def test_deterministic_across_calls_and_contexts(H, trees):
    t = trees["union3_general"]
    args = ((-0.47, -0.5, -0.43), (0.5, 0.44, 0.5), (96, 80, 88))
    a = t.extract_surface(*args, values=True)
    b = t.extract_surface(*args, values=True)
    ctx2 = H.Context(0)
    try:
        t2 = H.DeviceTree(ctx2, t.block)
        c = t2.extract_surface(*args, values=True)
        t2.close()
    finally:
        ctx2.close()
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_argument_errors_leave_the_context_usable(H, trees):
    t = trees["sphere"]
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    bad = [
        (ROOT_LO, (0.5, up, 0.5), (8, 8, 8), 0.0, "axis y"),
        ((-0.5, -0.5, -float(np.nextafter(np.float32(0.5), np.float32(1.0)))), ROOT_HI, (8, 8, 8), 0.0, "axis z"),
        (ROOT_LO, ROOT_HI, (8, 0, 8), 0.0, "axis y"),
        ((0.1, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, "axis x"),
        ((0.2, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, "axis x"),
        (ROOT_LO, ROOT_HI, (8, 8, 8), float("nan"), "iso"),
        (ROOT_LO, ROOT_HI, (8, 8, 8), float("inf"), "iso"),
        (ROOT_LO, ROOT_HI, (1024, 1024, 1024), 0.0, "2^30"),
    ]
    pts = np.random.default_rng(3).uniform(-0.5, 0.5, (1000, 3))  # (more than a host-answered call: the device path)
    want = t.query(pts)
    for lo, hi, n, iso, msg in bad:
        with pytest.raises(H.HpsdfError) as ei:
            t.extract_surface(lo, hi, n, iso)
        assert ei.value.status == 1 and msg in str(ei.value), (lo, hi, n, iso, str(ei.value))
        assert np.array_equal(t.query(pts), want)
    assert len(t.extract_surface(ROOT_LO, ROOT_HI, (8, 8, 8))[1]) > 0


@pytest.mark.parametrize("name", ["sphere", "union3_general"])
def test_round_trip_through_the_mesh_ingest(H, O, ctx, trees, name):
    """The extracted mesh (float32 vertices) passes the half-edge ingest (no HPSDF_ERR_OPEN_MESH), and the mesh field's sign is the
    tree's at points farther than 2 h from the level set -- except where the mesh field's own sign rule (the angle-weighted
    pseudo-normal of the closest feature, Mesh.cpp:162-242) misreads a sliver of the mesh: there the distance is still the tree's
    within 2 h and the CPU oracle's Mesh::SignedDistanceAtPt returns the very same value, i.e. the mesh is right and the sign is the
    reference's arithmetic.  Such points are held below 1 in 1000."""
    t = trees[name]
    lo, hi, n = (-0.4963, -0.4971, -0.4958), (0.4966, 0.4957, 0.4969), (90, 90, 90)
    verts, tris, vals = t.extract_surface(lo, hi, n, values=True)
    assert not np.any(vals == 0.0)
    v32 = verts.astype(np.float32)
    f = H.Field.mesh(ctx, v32, tris)  # raises HPSDF_ERR_OPEN_MESH if a half-edge has no twin
    try:
        h = max((hi[a] - lo[a]) / n[a] for a in range(3))
        rng = np.random.default_rng(11)
        p = rng.uniform(-0.49, 0.49, (20000, 3))
        q = t.query(p)
        keep = np.abs(q) > 2 * h
        p, q = p[keep], q[keep]
        m = f.eval(ctx, p)
        assert len(p) > 10000
        bad = np.sign(m) != np.sign(q)
        assert bad.sum() <= len(p) // 1000, bad.sum()
        if bad.any():
            assert np.all(np.abs(np.abs(m[bad]) - np.abs(q[bad])) <= 2 * h)
            om = O.MeshField(v32, tris).signed_distance(p[bad])[0].astype(np.float64)
            assert np.array_equal(om, m[bad])
    finally:
        f.close()


def test_cxx_extract_surface_on_gpu(H, tmp_path):
    exe = build_surface_prog(H, str(tmp_path))
    r = subprocess.run([exe, str(tmp_path / "s.obj")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    assert os.path.getsize(tmp_path / "s.obj") > 0
