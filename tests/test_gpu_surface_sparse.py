"""hpsdf_extract_surface_sparse on the device: bitwise the dense call's arrays wherever the dense call is allowed, the classification
kernel's bytes against the host version's, n = 2048 -- beyond the dense limit -- against dense windows and the sphere's topology, the
statistics, determinism, the empty result, argument errors, Octree.ExtractSurface(sparse=True) and the C++ drop-in's flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT_LO, ROOT_HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.3
SPHERE_TARGET = 1e-6


@pytest.fixture(scope="module")
def trees(H, ctx):
    out = {}
    for name, field, target in (("union3_top", H.Field.union3(), 1e-5), ("union3_general", H.Field.union3(), 1e-7),
                                ("sphere", H.Field.sphere(SPHERE_C, SPHERE_R), SPHERE_TARGET)):
        block, _ = H.create_block(ctx, H.make_config(target), field, 0)
        out[name] = H.DeviceTree(ctx, block)
    out["deep"] = H.DeviceTree(ctx, helpers.deep_chain_block(np.random.default_rng(5)))
    yield out
    for t in out.values():
        t.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# tests/test_gpu_surface.py's CASES restated (tree, lo, hi, n, iso; iso None: the median of the lattice values), one of them at a
# non-zero iso as well, and one near the dense call's limit
CASES = [
    ("union3_top", ROOT_LO, ROOT_HI, (48, 48, 48), 0.0),
    ("union3_general", ROOT_LO, ROOT_HI, (64, 64, 64), 0.0),
    ("union3_general", (-0.37, -0.41, -0.29), (0.23, 0.11, 0.31), (37, 64, 23), 0.0),  # off-centre, non-cubic
    ("union3_top", (-0.45, -0.3, -0.35), (0.4, 0.1, 0.05), (23, 41, 30), 0.0),
    ("deep", ROOT_LO, ROOT_HI, (40, 33, 47), None),
    ("deep", (0.2, 0.21, 0.19), (0.5, 0.5, 0.5), (45, 37, 41), None),  # the chain's corner: leaves down to depth 10
    ("sphere", ROOT_LO, ROOT_HI, (50, 50, 50), 0.0),
    ("sphere", ROOT_LO, ROOT_HI, (50, 50, 50), 0.05),
    ("union3_general", (-0.37, -0.41, -0.29), (0.23, 0.11, 0.31), (37, 64, 23), -0.011),
    ("union3_general", ROOT_LO, ROOT_HI, (1000, 1000, 1000), 0.0),  # 1001^3 points: just under the dense call's 2^30
]


def iso_of(t, lo, hi, n, iso):
    return float(np.median(t.query(S.lattice_points(lo, hi, n)))) if iso is None else iso


@pytest.mark.parametrize("name,lo,hi,n,iso", CASES)
def test_sparse_equals_dense_bit_for_bit(trees, name, lo, hi, n, iso):
    t = trees[name]
    iso = iso_of(t, lo, hi, n, iso)
    dv, dt = t.extract_surface(lo, hi, n, iso)
    sv, st, stats = t.extract_surface_sparse(lo, hi, n, iso, stats=True)
    print(name, n, iso, "verts", len(sv), "tris", len(st), stats)
    assert len(dt) > 0
    assert sv.shape == dv.shape and st.shape == dt.shape
    assert np.array_equal(bits(sv), bits(dv)), "vertex bits differ from the dense call's"
    assert np.array_equal(st, dt), "triangles differ from the dense call's"
    assert 0 < stats["active_blocks"] <= stats["blocks"] and stats["peak_scratch_bytes"] > 0


@pytest.mark.parametrize("name,lo,hi,n,iso", CASES)
def test_device_classes_equal_host_classes(H, trees, name, lo, hi, n, iso):
    t = trees[name]
    iso = iso_of(t, lo, hi, n, iso)
    dev = t.classify_surface_blocks(lo, hi, n, iso)
    host = H.surface_classify_host(t.block, lo, hi, n, iso)
    assert dev.shape == host.shape == (H.surface_block_count(n),)
    assert np.array_equal(dev, host), np.nonzero(dev != host)[0][:10]
    nb = len(host)
    assert np.array_equal(t.classify_surface_blocks(lo, hi, n, iso, first_block=nb // 3, count=nb // 2), host[nb // 3:nb // 3 + nb // 2])


N_BIG = 2048
H_BIG = 1.0 / N_BIG  # 2^-11: every lattice coordinate is an exact dyadic
WINDOW = 256


def dense_scratch_bytes(n):
    """What hpsdf_extract_surface's formula (csrc/surface.hip) asks for: values, bit words, their counts and prefixes, tile counts and prefixes."""
    pts, cubes = (n + 1) ** 3, n ** 3
    words, tiles = (3 * pts + 63) // 64, (cubes + 63) // 64
    return 8 * pts + 20 * words + 12 * tiles


def tri_rows(verts, tris):
    """a triangle as its three vertices' nine coordinates, bitwise -> sorted rows of 9 u64"""
    rows = bits(verts[tris.astype(np.int64)].reshape(len(tris), 9))
    return rows[np.lexsort(rows.T[::-1])]


@pytest.fixture(scope="module")
def big(H, trees):
    """the sparse meshes at n = 2048"""
    out = {}
    for name in ("sphere", "union3_general"):
        out[name] = trees[name].extract_surface_sparse(ROOT_LO, ROOT_HI, (N_BIG,) * 3, 0.0, stats=True)
    return out


def test_dense_refuses_2048_and_sparse_serves_it(H, trees, big):
    for name in ("sphere", "union3_general"):
        with pytest.raises(H.HpsdfError) as ei:
            trees[name].extract_surface(ROOT_LO, ROOT_HI, (N_BIG,) * 3)
        assert ei.value.status == 1 and "2^30" in str(ei.value)
        verts, tris, stats = big[name]
        print(name, "n = 2048: verts", len(verts), "tris", len(tris), stats)
        assert len(tris) > 0 and len(verts) > 0
        assert int(tris.max()) == len(verts) - 1


def test_sphere_at_2048_is_closed_with_euler_characteristic_2(big):
    verts, tris, _ = big["sphere"]
    V = len(verts)
    t = tris.astype(np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = np.minimum(e[:, 0], e[:, 1]) * V + np.maximum(e[:, 0], e[:, 1])  # (V^2 < 2^63)
    _, counts = np.unique(key, return_counts=True)
    assert counts.min() == 2 and counts.max() == 2, "an edge is not shared by exactly two triangles"
    # every directed edge once: consistent winding
    dkey = e[:, 0] * V + e[:, 1]
    assert len(np.unique(dkey)) == len(dkey)
    assert len(np.unique(t)) == V
    assert V - len(counts) + len(t) == 2


@pytest.mark.parametrize("name", ["sphere", "union3_general"])
def test_2048_equals_dense_windows(trees, big, name):
    """h = 2^-11 and every lattice coordinate is an exact dyadic, so a dense call on the sub-box [-0.5 + i0 h, -0.5 + (i0 + 256) h]^3
    with n = 256 has bitwise the same point coordinates and values: its triangles -- as coordinate triples -- must be the sparse
    mesh's triangles whose cube lies in the window.  (A triangle's cube: the one its centroid lies in; no triangle of the case table
    lies in a face of its cube.)"""
    verts, tris, _ = big[name]
    cen = verts[tris.astype(np.int64)].mean(axis=1)
    cube = np.floor((cen + 0.5) * N_BIG).astype(np.int64)
    compared = 0
    for pick in (0, len(verts) // 3, 2 * len(verts) // 3, len(verts) - 1):  # windows around vertices of the mesh: they cut the surface
        i0 = np.clip(np.floor((verts[pick] + 0.5) * N_BIG).astype(np.int64) - WINDOW // 2, 0, N_BIG - WINDOW)
        lo = tuple(-0.5 + float(i) * H_BIG for i in i0)
        hi = tuple(-0.5 + float(i + WINDOW) * H_BIG for i in i0)
        dv, dt = trees[name].extract_surface(lo, hi, (WINDOW,) * 3)
        inside = np.all((cube >= i0) & (cube < i0 + WINDOW), axis=1)
        print(name, "window", i0, "dense tris", len(dt), "sparse tris in it", int(inside.sum()))
        assert len(dt) == int(inside.sum())
        if len(dt) == 0:
            continue
        assert np.array_equal(tri_rows(dv, dt), tri_rows(verts, tris[inside]))
        compared += 1
    assert compared >= 3


def test_stats_at_2048(big):
    for name, (verts, tris, stats) in big.items():
        share = stats["active_blocks"] / stats["blocks"]
        print(name, "active share %.4f" % share, "peak scratch %.1f MiB" % (stats["peak_scratch_bytes"] / 2 ** 20),
              "dense formula %.1f MiB" % (dense_scratch_bytes(N_BIG) / 2 ** 20))
        assert stats["blocks"] == (N_BIG // 8) ** 3
        assert share < 0.05
        assert stats["peak_scratch_bytes"] < dense_scratch_bytes(N_BIG) / 20
        assert stats["leaves_visited"] >= stats["blocks"]
        assert stats["total_ms"] > 0 and all(stats[k] >= 0 for k in stats)


def test_deterministic_across_calls_and_contexts(H, trees):
    t = trees["union3_general"]
    args = ((-0.47, -0.5, -0.43), (0.5, 0.44, 0.5), (96, 80, 88))
    a = t.extract_surface_sparse(*args)
    b = t.extract_surface_sparse(*args)
    ctx2 = H.Context(0)
    try:
        t2 = H.DeviceTree(ctx2, t.block)
        c = t2.extract_surface_sparse(*args)
        t2.close()
    finally:
        ctx2.close()
    assert len(a[1]) > 0
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_an_iso_above_every_value_is_empty(H, ctx, trees):
    t = trees["sphere"]
    L = H.lib()
    lo3, hi3 = (C.c_double * 3)(*ROOT_LO), (C.c_double * 3)(*ROOT_HI)
    n3 = (C.c_uint32 * 3)(16, 16, 16)
    v, tr = C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)()
    nv, nt = C.c_uint64(7), C.c_uint64(7)
    st = H.SurfaceSparseStats()
    assert L.hpsdf_extract_surface_sparse(ctx.handle, t.handle, lo3, hi3, n3, 10.0, C.byref(v), C.byref(nv), C.byref(tr), C.byref(nt), C.byref(st)) == 0
    assert nv.value == 0 and nt.value == 0 and not v and not tr
    assert st.blocks == 8
    assert L.hpsdf_extract_surface_sparse(ctx.handle, t.handle, lo3, hi3, n3, 10.0, C.byref(v), C.byref(nv), C.byref(tr), C.byref(nt), None) == 0


def test_argument_errors_leave_the_context_usable(H, trees):
    t = trees["sphere"]
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    bad = [
        (ROOT_LO, (0.5, up, 0.5), (8, 8, 8), 0.0, "axis y"),
        ((-0.5, -0.5, -up), ROOT_HI, (8, 8, 8), 0.0, "axis z"),
        (ROOT_LO, ROOT_HI, (8, 0, 8), 0.0, "axis y"),
        ((0.1, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, "axis x"),
        ((0.2, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, "axis x"),
        (ROOT_LO, ROOT_HI, (8, 8, 8), float("nan"), "iso"),
        (ROOT_LO, ROOT_HI, (8, 8, 8), float("inf"), "iso"),
        (ROOT_LO, ROOT_HI, (1 << 20, 1 << 20, 1), 0.0, "2^40"),
        (ROOT_LO, ROOT_HI, ((1 << 20) + 1, 8, 8), 0.0, "2^20"),
    ]
    pts = np.random.default_rng(3).uniform(-0.5, 0.5, (1000, 3))
    want = t.query(pts)
    for lo, hi, n, iso, msg in bad:
        with pytest.raises(H.HpsdfError) as ei:
            t.extract_surface_sparse(lo, hi, n, iso)
        assert ei.value.status == 1 and msg in str(ei.value), (lo, hi, n, iso, str(ei.value))
        assert np.array_equal(t.query(pts), want)
    with pytest.raises(H.HpsdfError) as ei:
        t.classify_surface_blocks(ROOT_LO, ROOT_HI, (16, 16, 16), first_block=7, count=2)
    assert ei.value.status == 1 and "past" in str(ei.value)
    assert len(t.extract_surface(ROOT_LO, ROOT_HI, (8, 8, 8))[1]) > 0
    assert len(t.extract_surface_sparse(ROOT_LO, ROOT_HI, (8, 8, 8))[1]) > 0


def test_octree_extract_surface_sparse_flag(H):
    o = H.Octree()
    o.Create(H.make_config(1e-5), H.Field.sphere(SPHERE_C, SPHERE_R))
    args = ((-0.45, -0.4, -0.5), (0.5, 0.45, 0.42), (61, 50, 47), 0.01)
    dv, dt = o.ExtractSurface(*args)
    dv2, dt2 = o.ExtractSurface(*args, sparse=False)
    sv, st = o.ExtractSurface(*args, sparse=True)
    assert len(dt) > 0
    assert dv.tobytes() == dv2.tobytes() == sv.tobytes() and dt.tobytes() == dt2.tobytes() == st.tobytes()


CXX = r"""
#include "HP/Octree.h"
#include <cstdio>
#include <cstring>
int main() {
    try {
        SDF::Config cfg;
        cfg.targetErrorThreshold = 1e-4;
        cfg.continuity.enforce = false;
        SDF::Octree oct;
        oct.Create(cfg, SDF::DeviceField::Sphere(0.02, -0.01, 0.03, 0.3));
        const Eigen::Vector3i res(40, 36, 44);
        const SDF::SurfaceMesh d = oct.ExtractSurface(oct.GetRootAABB(), res);  // the existing calls: unchanged
        const SDF::SurfaceMesh d2 = oct.ExtractSurface(oct.GetRootAABB(), res, 0.0);
        const SDF::SurfaceMesh s = oct.ExtractSurface(oct.GetRootAABB(), res, 0.0, true);
        if (d.triangles.empty() || d2.triangles.size() != d.triangles.size()) { printf("empty\n"); return 2; }
        if (d.vertices.size() != s.vertices.size() || d.triangles.size() != s.triangles.size()) { printf("counts\n"); return 3; }
        if (std::memcmp(d.vertices.data(), s.vertices.data(), sizeof(d.vertices[0]) * d.vertices.size()) != 0) { printf("vertices\n"); return 4; }
        if (std::memcmp(d.triangles.data(), s.triangles.data(), sizeof(d.triangles[0]) * d.triangles.size()) != 0) { printf("triangles\n"); return 5; }
        printf("ok %zu %zu\n", s.vertices.size() / 3, s.triangles.size() / 3);
        return 0;
    } catch (const SDF::Error& e) {
        printf("SDF::Error %d: %s\n", e.status, e.what());
        return 1;
    }
}
"""


def build_sparse_prog(H, tmp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(tmp, "surface_sparse.cpp"), os.path.join(tmp, "surface_sparse")
    open(src, "w").write(CXX)
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(root, "include"), src, "-o", exe, "-L", libdir,
           "-lhpsdf", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def test_cxx_sparse_flag_on_gpu(H, tmp_path):
    exe = build_sparse_prog(H, str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
