"""QueryGradient on the GPU: the kernels (query_gradient.hip) against the device-free entry bit for bit -- every degree class, the
all-top-table kernel, the few-point kernel, the host-answered path, ragged last workgroups, both reduction orders --, built trees
against the long-double bound, out = NULL, ExtractSurface's normals, and a C++ caller of the drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hiprec as R
import hiprec_gradient as G
from conftest import ROOT
from helpers import edge_points, synthetic_block
from test_hiprec_cpu import ROOTS, _with_root, query_blocks

DBL_MAX = np.finfo(np.float64).max
SIZES = (1, 32, 33, 63, 64, 65, 4096 + 37)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _trees(rng):
    """query_blocks, an anisotropic root, and trees whose largest degree is 2 (all leaves in the top table; and not), 3, 5 and 12."""
    out = query_blocks(rng)
    out.append(("aniso", _with_root(synthetic_block(rng, [3, 5, 2, 7, 1, 4, 6, 0], 2), *ROOTS["aniso"])))
    out.append(("max2-top", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)))
    out.append(("max2", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 2, *ROOTS["cube"])))
    out.append(("max3", synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)))
    out.append(("max5", synthetic_block(rng, [5, 4, 3, 2, 1, 0, 5, 4], 2, *ROOTS["cube"])))
    out.append(("max12", synthetic_block(rng, [12, 7, 3, 2, 9, 0, 5, 6], 2)))
    return out


def _point_set(blk, rng):
    B = R.Block(blk)
    lo, hi = B.root_min.astype(np.float64), B.root_max.astype(np.float64)
    bad = lo + (hi - lo) * rng.uniform(0.0, 1.0, (64, 3))
    bad[:16, 0] = hi[0] + (hi[0] - lo[0]) * rng.uniform(0.01, 3.0, 16)
    bad[16:32, 1] = lo[1] - (hi[1] - lo[1]) * rng.uniform(0.01, 3.0, 16)
    bad[32:40] = np.nan
    bad[40:48, 2] = np.nan
    bad[48:56, 0] = np.inf
    bad[56:64] = -np.inf
    pts = np.concatenate([R.points_in_leaves(B, rng, 4096), B.from_unit(edge_points(rng)), bad])
    return pts[rng.permutation(len(pts))]


@pytest.mark.gpu
def test_device_equals_block_entry_bit_for_bit(H, ctx):
    rng = np.random.default_rng(71)
    degrees = set()
    try:
        for name, blk in _trees(rng):
            tree = H.DeviceTree(ctx, blk)
            degrees.add(tree.info()["max_degree"])
            pts = _point_set(blk, rng)
            for left in (0, 1):
                H.set_reduction_order(left)
                ctx.set_reduction_order(bool(left))
                for unit in (False, True):
                    wv, wg = H.query_gradient_block(blk, pts, unit=unit)
                    assert (wv == DBL_MAX).sum() >= 64 and np.isnan(wg[wv == DBL_MAX]).all()
                    for n in SIZES + (len(pts),):
                        v, g = tree.query_gradient(pts[:n], unit=unit)
                        assert np.array_equal(_bits(v), _bits(wv[:n])), (name, left, unit, n)
                        assert np.array_equal(_bits(g), _bits(wg[:n])), (name, left, unit, n)
                    # the kernels for the sizes the host answers itself: raw device arrays
                    for n in (1, 32, 33):
                        v, g = _device_call(H, ctx, tree, pts[:n], unit)
                        assert np.array_equal(_bits(v), _bits(wv[:n])) and np.array_equal(_bits(g), _bits(wg[:n])), (name, left, unit, n)
            tree.close()
    finally:
        ctx.set_reduction_order(None)
        H.set_reduction_order(0)
    assert {2, 3, 5, 12} <= degrees


def _device_call(H, ctx, tree, pts, unit, with_out=True):
    import torch
    n = len(pts)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_grad = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tree.query_gradient_device(d_pts.data_ptr(), n, d_out.data_ptr() if with_out else 0, d_grad.data_ptr(), unit=unit)
    ctx.synchronize()
    return d_out.cpu().numpy(), d_grad.cpu().numpy()


BUILT = {"union3_1e-5": ("union3", 1e-5, (-0.5,) * 3, (0.5,) * 3), "union3_1e-7": ("union3", 1e-7, (-0.5,) * 3, (0.5,) * 3),
         "sphere075_1e-6": ("sphere075", 1e-6, (-0.25,) * 3, (5.0,) * 3)}


def _built(H, ctx, case):
    from helpers import product_field
    field, target, rmin, rmax = BUILT[case]
    return H.create_block(ctx, H.make_config(target, rmin, rmax), product_field(H, field), 1024)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(BUILT))
def test_built_trees_within_the_bound(H, ctx, case):
    blk = _built(H, ctx, case)
    tree = H.DeviceTree(ctx, blk)
    if case == "union3_1e-5":
        info = tree.info()
        assert info["max_degree"] <= 2 and info["max_depth"] == 4          # the all-top-table shape
    rng = np.random.default_rng(73)
    pts = R.points_in_leaves(blk, rng, 2048)
    ref = G.gradient_reference(blk, pts, left=bool(ctx.reduction_order()))
    want = tree.query(pts)
    for unit in (False, True):
        v, g = tree.query_gradient(pts, unit=unit)
        assert np.array_equal(_bits(v), _bits(want)), case
        ex = G.excess(g, ref, unit)
        print(case, "unit" if unit else "world", "excess %.3g" % ex)
        assert ex <= 1, (case, unit, ex)
    bv, bg = H.query_gradient_block(blk, pts)
    v, g = tree.query_gradient(pts)
    assert np.array_equal(_bits(bv), _bits(v)) and np.array_equal(_bits(bg), _bits(g))
    tree.close()


@pytest.mark.gpu
def test_null_out_gives_the_same_gradients(H, ctx):
    rng = np.random.default_rng(79)
    for name, blk in (("chain", query_blocks(rng)[2][1]), ("max2-top", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1))):
        tree = H.DeviceTree(ctx, blk)
        pts = _point_set(blk, rng)
        for n in (5, 200, len(pts)):
            for unit in (False, True):
                v, g = _device_call(H, ctx, tree, pts[:n], unit)
                v0, g0 = _device_call(H, ctx, tree, pts[:n], unit, with_out=False)
                assert np.array_equal(_bits(g), _bits(g0)), (name, n, unit)
                assert (v0 == 7.0).all() and not (v == 7.0).any()
        # the host-array entry with out = NULL
        g1 = np.empty((len(pts), 3))
        H.check(H.lib().hpsdf_query_true_gradient_host(ctx.handle, tree.handle, pts.ctypes.data_as(C.c_void_p), len(pts), 0, None,
                                                       g1.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(_bits(g1), _bits(tree.query_gradient(pts)[1]))
        assert H.lib().hpsdf_query_true_gradient_host(ctx.handle, tree.handle, pts.ctypes.data_as(C.c_void_p), 4, 2, None,
                                                      g1.ctypes.data_as(C.c_void_p)) == 1
        assert H.lib().hpsdf_query_true_gradient_device(ctx.handle, tree.handle, None, 4, 0, None, None) == 1
        assert H.lib().hpsdf_query_true_gradient_device(ctx.handle, tree.handle, None, 0, 0, None, None) == 0
        tree.close()


@pytest.mark.gpu
def test_extract_surface_normals(H):
    o = H.Octree()
    o.Create(H.make_config(1e-5), H.Field.union3())
    lo, hi = (-0.5,) * 3, (0.5,) * 3
    verts, tris = o.ExtractSurface(lo, hi, 32)
    v2, t2, nrm = o.ExtractSurface(lo, hi, 32, normals=True)
    assert len(tris) > 0 and verts.tobytes() == v2.tobytes() and tris.tobytes() == t2.tobytes()
    want = o._tree.query_gradient(verts, unit=True)[1]
    assert nrm.shape == verts.shape and np.array_equal(_bits(nrm), _bits(want))
    assert (np.abs(np.sqrt((nrm.astype(R.LD) ** 2).sum(1)) - 1).astype(np.float64) <= 4 * R.U).all()
    sv, st, sn = o.ExtractSurface(lo, hi, 32, sparse=True, normals=True)
    assert sv.tobytes() == verts.tobytes() and st.tobytes() == tris.tobytes() and np.array_equal(_bits(sn), _bits(nrm))
    val, g = o.QueryGradient((0.1, -0.2, 0.3))
    assert isinstance(val, float) and g.shape == (3,) and val == o.Query((0.1, -0.2, 0.3))
    vals, gs = o.QueryGradient(np.array([[0.1, -0.2, 0.3], [2.0, 0.0, 0.0]]), unit=True)
    assert vals[1] == DBL_MAX and np.isnan(gs[1]).all() and abs(float(np.sqrt((gs[0].astype(R.LD) ** 2).sum())) - 1) <= 4 * R.U


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/query_gradient_caller.cpp through include/hpsdf_octree.hpp: QueryGradient scalar and batched, SurfaceNormals --
    the bits it prints are the Python binding's."""
    from helpers import product_field
    blk = H.create_block(ctx, H.make_config(1e-5), product_field(H, "union3"), 1024)[0]
    rng = np.random.default_rng(83)
    pts = rng.uniform(-0.5, 0.5, (300, 3))
    pts[::37] *= 3.0
    pts[5] = np.nan
    exe = str(tmp_path / "query_gradient_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "query_gradient_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
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
        rows.setdefault(f[0], []).append([int(f[1]), int(f[2])] if f[0] == "M" else [int(x, 16) for x in f[2:]])
    hexrows = lambda k: np.array(rows[k], np.uint64)
    bv, bg = H.query_gradient_block(blk, pts)
    uv, ug = H.query_gradient_block(blk, pts, unit=True)
    B, U = hexrows("B"), hexrows("U")
    assert np.array_equal(B[:, 0], _bits(bv)) and np.array_equal(B[:, 1:], _bits(bg))
    assert np.array_equal(U[:, 0], _bits(uv)) and np.array_equal(U[:, 1:], _bits(ug))
    S = hexrows("S")
    assert len(S) == 40
    for i in range(40):
        assert S[i, 0] == _bits(bv)[i] and np.array_equal(S[i, 1:], _bits(ug if i % 2 else bg)[i]), i
    o = H.Octree()
    o.FromMemoryBlock(blk)
    verts, tris, nrm = o.ExtractSurface((-0.5,) * 3, (0.5,) * 3, 24, normals=True)
    assert rows["M"][0] == [len(verts), len(tris)] and len(verts) > 0
    assert np.array_equal(hexrows("V"), _bits(verts)) and np.array_equal(hexrows("N"), _bits(nrm))
