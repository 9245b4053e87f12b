"""ExtractSurfaceDual on the device: hpsdf_extract_surface_dual against hpsdf_extract_surface_dual_block (the same statements on the
calling thread, which tests/test_surface_dual_cpu.py holds to the restatement) bit for bit -- vertices, triangles, info bytes and
lattice values -- on built and uploaded trees of every degree class and on lattices from one cube to a few waves of cubes; the
sharp-feature assertions on the box through the device path; the Python and C++ front ends."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import surface_reference as S
from conftest import ROOT
from helpers import synthetic_block
from test_surface_dual_cpu import BOX_C, BOX_H, BOX_LO, BOX_N, SPHERE_C, SPHERE_R, box_checks

pytestmark = pytest.mark.gpu

LATTICES = [(1, 1, 1), (2, 2, 2), (1, 17, 8), (16, 9, 1), (8, 8, 8), (9, 8, 7), (7, 9, 16), (65, 2, 2)]
ROOT_LO, ROOT_HI = (-0.5,) * 3, (0.5,) * 3


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def trees(H, ctx):
    """name -> (tree, lo, hi): the sphere at 1e-6 (every leaf in the top table), the box at 1e-7, union3 at 1e-7 (degrees to 5 and
    beyond: the any-tree gradient path) and two synthetic blocks uploaded (largest degree 3 and 12)."""
    rng = np.random.default_rng(223)
    out = {}
    built = {"sphere": (H.Field.sphere(tuple(SPHERE_C), SPHERE_R), 1e-6, SPHERE_C - 0.35, SPHERE_C + 0.35),
             "box": (H.Field.analytic([(H.PRIM_BOX, H.OP_UNION, list(BOX_C) + list(BOX_H))]), 1e-7, BOX_LO, BOX_LO + 0.75),
             "union3": (H.Field.union3(), 1e-7, np.array([-0.43, -0.41, -0.45]), np.array([0.37, 0.39, 0.33]))}
    for name, (field, target, lo, hi) in built.items():
        out[name] = (H.DeviceTree(ctx, H.create_block(ctx, H.make_config(target), field, 0)[0]), lo, hi)
    for name, degrees in (("max3", [3, 2, 1, 0, 3, 3, 2, 1]), ("max12", [12, 7, 3, 2, 9, 0, 5, 6])):
        out[name] = (H.DeviceTree(ctx, synthetic_block(rng, degrees, 2)), np.full(3, -0.469), np.full(3, 0.453))
    yield out
    for t, _, _ in out.values():
        t.close()


def assert_same(dev, host, what):
    for name, d, h in zip(("verts", "tris", "info", "values"), dev, host):
        assert d.shape == h.shape and d.dtype == h.dtype, (what, name, d.shape, h.shape)
        assert np.array_equal(np.ascontiguousarray(d).view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), (what, name)


@pytest.mark.parametrize("name", ["sphere", "box", "union3", "max3", "max12"])
def test_device_call_equals_the_block_entry_bit_for_bit(H, trees, name):
    t, lo, hi = trees[name]
    seen = 0
    for n in LATTICES:
        vals = t.extract_surface_dual(lo, hi, n, values=True)[2]
        for iso, tau in ((0.0, 0.1), (float(np.median(vals)), 0.0), (float(np.median(vals)), 0.5)):
            dev = t.extract_surface_dual(lo, hi, n, iso, tau, values=True, info=True)
            host = H.extract_surface_dual_block(t.block, lo, hi, n, iso, tau, values=True, info=True)
            assert_same(dev, host, (name, n, iso, tau))
            seen += len(dev[0])
    print(name, "vertices compared:", seen)
    assert seen > 0


def test_medium_lattice_on_union3(H, trees):
    """(48, 40, 33): 63 360 cubes -- many workgroups, words whose cubes and edges straddle rows and slabs."""
    t, lo, hi = trees["union3"]
    n = (48, 40, 33)
    dev = t.extract_surface_dual(lo, hi, n, 0.0, 0.1, values=True, info=True)
    host = H.extract_surface_dual_block(t.block, lo, hi, n, 0.0, 0.1, values=True, info=True)
    assert_same(dev, host, "union3 medium")
    verts, tris, info, vals = dev
    mc_v, mc_t = t.extract_surface(lo, hi, n, 0.0)
    print("V %d T %d, marching cubes V %d T %d, ranks %s, timings %s" % (len(verts), len(tris), len(mc_v), len(mc_t),
                                                                       np.bincount(info & 3, minlength=4).tolist(), H.surface_dual_last_timings()))
    # union3 lies inside this box: the mesh is closed -- every directed edge has its reverse as often as it occurs -- and what
    # unmatched_edges reports are edges that occur more than once, the non-manifold edges of ambiguous faces where the primitives meet
    e = Counter(map(tuple, S.directed_edges(tris).tolist()))
    assert len(verts) > 1000 and all(e.get((b, a), 0) == c for (a, b), c in e.items())
    assert all(e[k] > 1 for k in S.unmatched_edges(tris))
    ms = H.surface_dual_last_timings()
    assert set(ms) == {"lattice", "ballots", "scan", "hermite", "vertices", "quads", "d2h", "total"} and ms["total"] > 0


def test_box_keeps_its_corners_through_the_device_path(H, trees):
    """Assertions (a)-(e) of tests/test_surface_dual_cpu.py's sharp-feature test on the device's mesh of the device-built box."""
    t, lo, hi = trees["box"]
    verts, tris, info, vals = t.extract_surface_dual(lo, hi, BOX_N, 0.0, 0.1, values=True, info=True)
    mc_verts, _ = t.extract_surface(lo, hi, BOX_N, 0.0)
    m = box_checks(H, verts, tris, info, mc_verts)
    print("corner -> dual %.4f..%.4f h, -> marching cubes %.3f..%.3f h, surface %.4f h, volume %.3f %%"
          % (m["dual"].min(), m["dual"].max(), m["mc"].min(), m["mc"].max(), m["surface"], 100 * m["volume"]))


def test_octree_front_end_composes_with_normals_and_curvature(H, trees):
    t, lo, hi = trees["sphere"]
    o = H.Octree()
    o.FromMemoryBlock(t.block)
    n = (9, 8, 7)
    verts, tris = o.ExtractSurface(lo, hi, n, dual=True)
    want = o._tree.extract_surface_dual(lo, hi, n, 0.0, 0.1)
    assert np.array_equal(bits(verts), bits(want[0])) and np.array_equal(tris, want[1]) and len(tris) > 0
    v2, t2, normals = o.ExtractSurface(lo, hi, n, dual=True, normals=True)
    assert np.array_equal(bits(v2), bits(verts)) and np.array_equal(t2, tris)
    assert np.array_equal(bits(normals), bits(o._tree.query_gradient(verts, unit=True)[1]))
    v3, t3, n3, curv = o.ExtractSurface(lo, hi, n, dual=True, normals=True, curvature=True, tau=0.1)
    assert np.array_equal(bits(v3), bits(verts)) and np.array_equal(bits(n3), bits(normals)) and curv.shape == (len(verts), 2)
    other = o.ExtractSurface(lo, hi, n, dual=True, tau=0.0)[0]
    assert other.shape == verts.shape and not np.array_equal(bits(other), bits(verts))  # tau reaches the call
    mc = o.ExtractSurface(lo, hi, n)
    assert np.array_equal(bits(mc[0]), bits(o._tree.extract_surface(lo, hi, n)[0])) and mc[0].shape != verts.shape  # the default is still marching cubes
    with pytest.raises(ValueError):
        o.ExtractSurface(lo, hi, n, dual=True, sparse=True)
    o.Clear()


def test_context_under_reduction_order_1_matches_the_block_entry_under_it(H, trees):
    t, lo, hi = trees["union3"]
    c2 = H.Context(0)
    before = H.reduction_order()
    try:
        c2.set_reduction_order(1)
        t2 = H.DeviceTree(c2, t.block)
        n = (16, 9, 5)
        dev = t2.extract_surface_dual(lo, hi, n, 0.0, 0.1, values=True, info=True)
        H.set_reduction_order(1)
        host1 = H.extract_surface_dual_block(t.block, lo, hi, n, 0.0, 0.1, values=True, info=True)
        H.set_reduction_order(0)
        host0 = H.extract_surface_dual_block(t.block, lo, hi, n, 0.0, 0.1, values=True, info=True)
        assert_same(dev, host1, "order 1")
        print("vertices whose bits depend on the order:", int((bits(host0[0]) != bits(host1[0])).any(axis=1).sum()), "of", len(host0[0]))
        t2.close()
    finally:
        H.set_reduction_order(before)
        c2.close()


CXX = r'''
#include "HP/Octree.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {
    try {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        std::vector<char> buf(size);
        if (fread(buf.data(), 1, size, f) != (size_t)size) return 3;
        fclose(f);
        SDF::Octree oct;
        MemoryBlock blk;
        blk.size = (usize)size, blk.ptr = buf.data();
        oct.FromMemoryBlock(blk);
        Eigen::AlignedBox3f area(Eigen::Vector3f(-0.375f, -0.40625f, -0.4375f), Eigen::Vector3f(0.375f, 0.34375f, 0.3125f));
        const SDF::SurfaceMesh m = oct.ExtractSurfaceDual(area, Eigen::Vector3i(16, 9, 5), 0.0, 0.25);
        const SDF::SurfaceMesh d = oct.ExtractSurfaceDual(area, Eigen::Vector3i(16, 9, 5));
        if (m.vertices.size() != d.vertices.size() || m.triangles != d.triangles) { printf("default tau changes the topology\n"); return 4; }
        FILE* o = fopen(argv[2], "wb");
        const unsigned long long nv = m.vertices.size() / 3, nt = m.triangles.size() / 3;
        fwrite(&nv, 8, 1, o), fwrite(&nt, 8, 1, o);
        fwrite(m.vertices.data(), 8, m.vertices.size(), o);
        fwrite(m.triangles.data(), sizeof(m.triangles[0]), m.triangles.size(), o);
        fclose(o);
        printf("ok %llu %llu %zu\n", nv, nt, sizeof(m.triangles[0]));
        return 0;
    } catch (const SDF::Error& e) {
        printf("SDF::Error %d: %s\n", e.status, e.what());
        return e.status == HPSDF_ERR_NO_DEVICE ? 42 : 1;
    }
}
'''


def test_cxx_caller_returns_the_python_calls_mesh(H, trees, tmp_path):
    """One hpsdf_octree.hpp caller of ExtractSurfaceDual, compiled as tests/test_cxx_dropin.py compiles its programs."""
    t, _, _ = trees["union3"]
    src, exe, blk, out = (str(tmp_path / x) for x in ("dual.cpp", "dual", "tree.bin", "mesh.bin"))
    open(src, "w").write(CXX)
    open(blk, "wb").write(bytes(t.block))
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir,
           "-lhpsdf", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, blk, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    nv, nt = (int(x) for x in np.frombuffer(raw[:16], np.uint64))
    index_bytes = int(r.stdout.split()[3])
    verts = np.frombuffer(raw[16:16 + 24 * nv], np.float64).reshape(nv, 3)
    tris = np.frombuffer(raw[16 + 24 * nv:], {4: np.uint32, 8: np.uint64}[index_bytes]).reshape(nt, 3)
    lo, hi = (-0.375, -0.40625, -0.4375), (0.375, 0.34375, 0.3125)   # exact in float32: the C++ box is float
    want = t.extract_surface_dual(lo, hi, (16, 9, 5), 0.0, 0.25)
    assert nv == len(want[0]) > 0 and nt == len(want[1]) > 0
    assert np.array_equal(bits(verts), bits(want[0])) and np.array_equal(tris.astype(np.uint64), want[1])
