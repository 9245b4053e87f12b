"""ProjectToSurface on the GPU: the kernels (project.hip) against the device-free entry bit for bit -- every degree class, the
all-top-table shape, the few-point kernel, the host-answered path, ragged last workgroups, both reduction orders, the optional outputs,
the in-place call --, built trees, ExtractSurface(project=True) against the restated acceptance rule, and a C++ caller of the drop-in."""
import os
import subprocess

import numpy as np
import pytest

import hiprec as R
import project_reference as P
from conftest import ROOT
from test_gpu_query_gradient import BUILT, _built, _point_set, _trees
from test_project_cpu import assert_rows_equal, levels

SIZES = (1, 32, 33, 63, 64, 65, 4096 + 37)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device_call(H, ctx, tree, pts, iso, tol, max_iter, unit, optional=True, in_place=False):
    """hpsdf_project_device on raw device arrays -> the five arrays (the optional ones keep their fill of 7 when not passed)."""
    import torch
    n = len(pts)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_xyz = d_pts if in_place else torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    d_val = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_grad = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    d_it = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    opt = [t.data_ptr() if optional else 0 for t in (d_val, d_grad, d_it, d_st)]
    tree.project_device(d_pts.data_ptr(), n, d_xyz.data_ptr(), *opt, iso=iso, tol=tol, max_iter=max_iter, unit=unit)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in (d_xyz, d_val, d_grad, d_it, d_st))


@pytest.mark.gpu
def test_device_equals_block_entry_bit_for_bit(H, ctx):
    rng = np.random.default_rng(211)
    degrees, seen = set(), set()
    try:
        for name, blk in _trees(rng):
            tree = H.DeviceTree(ctx, blk)
            degrees.add(tree.info()["max_degree"])
            pts = _point_set(blk, rng)
            _, tol = levels(H, blk, pts)
            for left in (0, 1):
                H.set_reduction_order(left)
                ctx.set_reduction_order(bool(left))
                for unit in (False, True):
                    for max_iter in (0, 8):
                        what = (name, left, unit, max_iter)
                        want = H.project_block(blk, pts, 0.0, tol, max_iter, unit)
                        seen |= set(int(s) for s in np.unique(want[4]))
                        for n in SIZES + (len(pts),):
                            assert_rows_equal(tree.project(pts[:n], 0.0, tol, max_iter, unit), [w[:n] for w in want], what + (n,))
                        # the kernels for the sizes the host answers itself: raw device arrays, with and without the optional outputs
                        for n in (1, 32, 33):
                            got = _device_call(H, ctx, tree, pts[:n], 0.0, tol, max_iter, unit)
                            assert_rows_equal(got, [w[:n] for w in want], what + (n, "device"))
                            bare = _device_call(H, ctx, tree, pts[:n], 0.0, tol, max_iter, unit, optional=False)
                            assert np.array_equal(_bits(bare[0]), _bits(want[0][:n])), what + (n, "no optional outputs")
                            assert all((b == 7).all() for b in bare[1:])
                        for n in (33, len(pts)):
                            got = _device_call(H, ctx, tree, pts[:n], 0.0, tol, max_iter, unit, in_place=True)
                            assert_rows_equal(got, [w[:n] for w in want], what + (n, "in place"))
            tree.close()
    finally:
        ctx.set_reduction_order(None)
        H.set_reduction_order(0)
    assert {2, 3, 5, 12} <= degrees and seen == {0, 1, 2, 3}


@pytest.mark.gpu
def test_argument_checks_on_the_context_entries(H, ctx):
    import ctypes as C
    rng = np.random.default_rng(223)
    blk = _trees(rng)[0][1]
    tree = H.DeviceTree(ctx, blk)
    pts = _point_set(blk, rng)[:40].copy()
    out = np.full((40, 3), 7.0)
    st = np.full(40, 7, np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = H.lib()
    host = lambda t, n, iso, tol, mi, fl, o: L.hpsdf_project_host(ctx.handle, t, vp(pts), n, iso, tol, mi, fl, vp(o), None, None, None, vp(st))
    for n in (4, 40):      # the host-answered size and one that would reach the device
        assert host(tree.handle, n, 0.0, 1e-9, 16, 2, out) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, 0.0, -1.0, 16, 0, out) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, 0.0, float("nan"), 16, 0, out) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, float("inf"), 1e-9, 16, 0, out) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, 0.0, 1e-9, 256, 0, out) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, 0.0, 1e-9, 16, 0, None) == H.ERR_INVALID_ARGUMENT
        assert host(None, n, 0.0, 1e-9, 16, 0, out) == H.ERR_INVALID_ARGUMENT
        assert (out == 7.0).all() and (st == 7).all()
    assert host(tree.handle, 0, 0.0, 1e-9, 16, 0, None) == H.OK
    assert L.hpsdf_project_device(ctx.handle, tree.handle, None, 4, 0.0, 1e-9, 16, 0, None, None, None, None, None) == H.ERR_INVALID_ARGUMENT
    assert L.hpsdf_project_device(ctx.handle, tree.handle, None, 0, 0.0, 1e-9, 16, 0, None, None, None, None, None) == H.OK
    h3 = (C.c_double * 3)(0.1, 0.1, 0.1)
    moved = C.c_uint64(77)
    spv = L.hpsdf_surface_project_vertices
    assert spv(ctx.handle, tree.handle, vp(out), 40, None, 0.0, 1e-9, 16, C.byref(moved)) == H.ERR_INVALID_ARGUMENT
    assert spv(ctx.handle, tree.handle, None, 40, h3, 0.0, 1e-9, 16, C.byref(moved)) == H.ERR_INVALID_ARGUMENT
    assert spv(ctx.handle, tree.handle, vp(out), 40, (C.c_double * 3)(0.1, -0.1, 0.1), 0.0, 1e-9, 16, C.byref(moved)) == H.ERR_INVALID_ARGUMENT
    assert spv(ctx.handle, tree.handle, vp(out), 40, h3, 0.0, 1e-9, 300, C.byref(moved)) == H.ERR_INVALID_ARGUMENT
    assert (out == 7.0).all() and moved.value == 77
    assert spv(ctx.handle, tree.handle, None, 0, h3, 0.0, 1e-9, 16, C.byref(moved)) == H.OK and moved.value == 0
    tree.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union3_1e-5", "union3_1e-7"])
def test_built_trees(H, ctx, case):
    """Device equals block on trees Create built, and the iteration does its work there: at most 3 % of 2048 uniform points end at
    the iteration limit (the restatement gave 0.76 % on union3 at 1e-5 -- points that hop across the creases of the union; the cap
    only keeps a kernel that gives up everywhere from passing)."""
    blk = _built(H, ctx, case)
    tree = H.DeviceTree(ctx, blk)
    rng = np.random.default_rng(227)
    pts = R.points_in_leaves(blk, rng, 2048)
    got = tree.project(pts, 0.0, 1e-9, 16)
    assert_rows_equal(got, H.project_block(blk, pts, 0.0, 1e-9, 16), case)
    counts = np.bincount(got[4], minlength=4)
    print(case, "status counts", counts.tolist(), "mean evaluations %.2f" % (got[3].astype(np.float64) + 1).mean())
    assert counts[P.ITER_LIMIT] <= 0.03 * len(pts), counts
    assert counts[P.CONVERGED] > 0
    conv = got[4] == P.CONVERGED
    assert (np.abs(got[1][conv]) <= 1e-9).all()
    tree.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union3", "sphere"])
def test_extract_surface_project(H, case):
    o = H.Octree()
    if case == "union3":
        o.Create(H.make_config(1e-5), H.Field.union3())
    else:
        o.Create(H.make_config(1e-8), H.Field.sphere())
    lo, hi, tol = (-0.5,) * 3, (0.5,) * 3, 1e-9
    h = H.surface_cube_size(lo, hi, (32,) * 3)
    assert h == (1.0 / 32,) * 3
    for sparse in (False, True):
        verts, tris = o.ExtractSurface(lo, hi, 32, sparse=sparse)
        pv, pt = o.ExtractSurface(lo, hi, 32, sparse=sparse, project=True)
        assert len(tris) > 0 and pt.tobytes() == tris.tobytes() and pv.shape == verts.shape
        rows = H.project_block(o.block, verts, 0.0, tol, 16)
        want, n_moved = P.accept_vertices(verts, rows[0], rows[4], h)
        assert np.array_equal(_bits(pv), _bits(want)), (case, sparse)
        moved = (_bits(pv) != _bits(verts)).any(1)
        assert n_moved > 0 and moved.any() and o._tree.project_vertices(verts, h)[1] == n_moved
        assert (np.abs(pv - verts) <= 0.5 * np.asarray(h)).all()
        before, after = np.abs(o.Query(verts)), np.abs(o.Query(pv))
        print(case, "sparse" if sparse else "dense", "%d of %d vertices moved; max |Query| %.3g -> %.3g over the moved ones; largest move %.3g of a cube"
              % (n_moved, len(verts), before[moved].max(), after[moved].max(), (np.abs(pv - verts) / np.asarray(h)).max()))
        if case == "sphere":
            assert before[moved].max() > 1e-5 and after[moved].max() <= tol
        nv, nt, nrm = o.ExtractSurface(lo, hi, 32, sparse=sparse, normals=True, project=True)
        assert nv.tobytes() == pv.tobytes() and nt.tobytes() == tris.tobytes()
        assert np.array_equal(_bits(nrm), _bits(o._tree.query_gradient(pv, unit=True)[1]))
    p, val, g, it, st = o.ProjectToSurface((0.1, -0.2, 0.3))
    assert p.shape == (3,) and g.shape == (3,) and isinstance(val, float) and isinstance(it, int) and isinstance(st, int)
    assert (val, ) == (o.Query(p),)
    many = o.ProjectToSurface(np.array([[0.1, -0.2, 0.3], [2.0, 0.0, 0.0]]), unit=True)
    assert many[4][1] == P.LEFT_ROOT and np.array_equal(many[0][1], [2.0, 0.0, 0.0]) and np.isnan(many[2][1]).all()
    assert np.array_equal(_bits(many[0][0]), _bits(p)) and int(many[4][0]) == st


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/project_caller.cpp through include/hpsdf_octree.hpp: ProjectToSurface scalar and batched, ProjectSurface -- the bits
    it prints are the Python binding's."""
    from helpers import product_field
    blk = H.create_block(ctx, H.make_config(1e-5), product_field(H, "union3"), 1024)[0]
    rng = np.random.default_rng(229)
    pts = rng.uniform(-0.5, 0.5, (300, 3))
    pts[::37] *= 3.0
    pts[5] = np.nan
    exe = str(tmp_path / "project_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "project_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    (tmp_path / "blk.bin").write_bytes(blk)
    (tmp_path / "pts.bin").write_bytes(np.ascontiguousarray(pts).tobytes())
    r = subprocess.run([exe, str(tmp_path / "blk.bin"), str(tmp_path / "pts.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "M":
            rows["M"] = [int(x) for x in f[1:]]
        elif f[0] == "V":
            rows.setdefault("V", []).append([int(x, 16) for x in f[2:]])
        else:
            rows.setdefault(f[0], []).append([int(f[2]), int(f[3])] + [int(x, 16) for x in f[4:]])

    def check(tag, want, count):
        got = np.array(rows[tag], np.uint64)
        assert len(got) == count
        assert np.array_equal(got[:, 0], want[4][:count]) and np.array_equal(got[:, 1], want[3][:count]), tag
        assert np.array_equal(got[:, 2:5], _bits(want[0])[:count]) and np.array_equal(got[:, 5], _bits(want[1])[:count]), tag
        assert np.array_equal(got[:, 6:9], _bits(want[2])[:count]), tag

    world, unit = H.project_block(blk, pts, 0.0, 1e-9, 16), H.project_block(blk, pts, 0.0, 1e-9, 16, True)
    check("B", world, len(pts))
    check("U", unit, len(pts))
    mixed = [np.where((np.arange(len(pts)) % 2 == 1).reshape((-1,) + (1,) * (w.ndim - 1)), u, w) for w, u in zip(world, unit)]
    check("S", mixed, 40)
    o = H.Octree()
    o.FromMemoryBlock(blk)
    verts, tris = o.ExtractSurface((-0.5,) * 3, (0.5,) * 3, 24)
    pv, n_moved = o._tree.project_vertices(verts, H.surface_cube_size((-0.5,) * 3, (0.5,) * 3, (24,) * 3))
    assert rows["M"] == [len(verts), len(tris), n_moved] and n_moved > 0
    assert np.array_equal(np.array(rows["V"], np.uint64), _bits(pv))
