"""QueryHessian on the GPU: the kernels (query_hessian.hip) against the device-free entry bit for bit -- every degree class, the
few-point kernel, the host-answered path, ragged last workgroups, both reduction orders, unit and curvature on and off --, NULL
outputs, built trees against the long-double bound, ExtractSurface's curvature, and a C++ caller of the drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hiprec as R
import hiprec_hessian as HS
from conftest import ROOT
from test_gpu_query_gradient import _point_set, _trees

DBL_MAX = np.finfo(np.float64).max
SIZES = (1, 32, 33, 63, 64, 65, 4096 + 37)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, n, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(g), _bits(w[:n])), what + (k,)


def _device_call(H, ctx, tree, pts, unit, mask=15):
    """hpsdf_query_hessian_device on raw device arrays filled with 7.0; bit k of mask: output k (out, grad, hess, curv) is passed."""
    import torch
    n = len(pts)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    bufs = [torch.full(shape, 7.0, dtype=torch.float64, device="cuda") for shape in ((n,), (n, 3), (n, 6), (n, 2))]
    torch.cuda.synchronize()
    tree.query_hessian_device(d_pts.data_ptr(), n, *[b.data_ptr() if mask >> k & 1 else 0 for k, b in enumerate(bufs)], unit=unit)
    ctx.synchronize()
    return [b.cpu().numpy() for b in bufs]


@pytest.mark.gpu
def test_device_equals_block_entry_bit_for_bit(H, ctx):
    rng = np.random.default_rng(271)
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
                    want = H.query_hessian_block(blk, pts, unit=unit, curvature=True)
                    bad = want[0] == DBL_MAX
                    assert bad.sum() >= 64 and all(np.isnan(w[bad]).all() for w in want[1:])
                    for curvature in (False, True):
                        for n in SIZES + (len(pts),):
                            got = tree.query_hessian(pts[:n], unit=unit, curvature=curvature)
                            assert len(got) == 3 + curvature
                            _same(got, want, n, (name, left, unit, curvature, n))
                        # the kernels for the sizes the host answers itself: raw device arrays
                        for n in (1, 32, 33):
                            got = _device_call(H, ctx, tree, pts[:n], unit, 15 if curvature else 7)
                            _same(got[:3 + curvature], want, n, (name, left, unit, curvature, n, "raw"))
                            assert curvature or (got[3] == 7.0).all()
            tree.close()
    finally:
        ctx.set_reduction_order(None)
        H.set_reduction_order(0)
    assert {2, 3, 5, 12} <= degrees


@pytest.mark.gpu
def test_null_outputs_stay_untouched(H, ctx):
    rng = np.random.default_rng(277)
    trees = dict(_trees(rng))
    for name in ("chain", "max2-top", "max12"):
        blk = trees[name]
        tree = H.DeviceTree(ctx, blk)
        pts = _point_set(blk, rng)
        for n in (5, 200, len(pts)):
            full = _device_call(H, ctx, tree, pts[:n], True)
            assert not any((b == 7.0).all() for b in full)
            for mask in range(16):
                if not mask & 12:       # hess and curv both NULL: refused, nothing written
                    continue
                got = _device_call(H, ctx, tree, pts[:n], True, mask)
                for k in range(4):
                    if mask >> k & 1:
                        assert np.array_equal(_bits(got[k]), _bits(full[k])), (name, n, mask, k)
                    else:
                        assert (got[k] == 7.0).all(), (name, n, mask, k)
        # the host-array entry with NULL outputs, above the size the host answers itself
        curv = np.full((len(pts), 2), 7.0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        H.check(H.lib().hpsdf_query_hessian_host(ctx.handle, tree.handle, vp(pts), len(pts), 0, None, None, None, vp(curv)))
        assert np.array_equal(_bits(curv), _bits(tree.query_hessian(pts, curvature=True)[3]))
        assert np.array_equal(_bits(curv), _bits(tree.query_curvature(pts)))
        hess = np.full((4, 6), 7.0)
        lib = H.lib()
        assert lib.hpsdf_query_hessian_host(ctx.handle, tree.handle, vp(pts), 4, 2, None, None, vp(hess), None) == H.ERR_INVALID_ARGUMENT
        assert lib.hpsdf_query_hessian_host(ctx.handle, tree.handle, vp(pts), 4, 0, vp(curv), vp(curv), None, None) == H.ERR_INVALID_ARGUMENT
        assert lib.hpsdf_query_hessian_host(ctx.handle, None, vp(pts), 4, 0, None, None, vp(hess), None) == H.ERR_INVALID_ARGUMENT
        assert lib.hpsdf_query_hessian_device(ctx.handle, tree.handle, None, 4, 0, None, None, vp(hess), None) == H.ERR_INVALID_ARGUMENT
        assert lib.hpsdf_query_hessian_device(ctx.handle, tree.handle, vp(pts), 4, 0, None, None, None, None) == H.ERR_INVALID_ARGUMENT
        assert lib.hpsdf_query_hessian_device(ctx.handle, tree.handle, None, 0, 0, None, None, vp(hess), None) == H.OK
        assert (hess == 7.0).all()
        tree.close()


BUILT = {"union3_1e-7": ("union3", 1e-7, (-0.5,) * 3, (0.5,) * 3), "sphere075_1e-6": ("sphere075", 1e-6, (-0.25,) * 3, (5.0,) * 3)}
_built_blocks = {}


def _built(H, ctx, case):
    from helpers import product_field
    if case not in _built_blocks:
        field, target, rmin, rmax = BUILT[case]
        _built_blocks[case] = H.create_block(ctx, H.make_config(target, rmin, rmax), product_field(H, field), 1024)[0]
    return _built_blocks[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(BUILT))
def test_built_trees_within_the_bound(H, ctx, case):
    blk = _built(H, ctx, case)
    tree = H.DeviceTree(ctx, blk)
    rng = np.random.default_rng(281)
    pts = R.points_in_leaves(blk, rng, 512)
    ref = HS.hessian_reference(blk, pts, left=bool(ctx.reduction_order()))
    v, g, hs, cv = tree.query_hessian(pts, curvature=True)
    assert np.array_equal(_bits(v), _bits(tree.query(pts))), case
    assert np.array_equal(_bits(g), _bits(tree.query_gradient(pts)[1])), case
    ex = HS.excess(hs, ref)
    print(case, "max degree %d, excess %.3g" % (tree.info()["max_degree"], ex))
    assert ex <= 1, (case, ex)
    _same((v, g, hs, cv), H.query_hessian_block(blk, pts, curvature=True), len(pts), (case,))
    tree.close()


@pytest.mark.gpu
def test_extract_surface_curvature(H):
    o = H.Octree()
    o.Create(H.make_config(1e-5), H.Field.union3())
    lo, hi = (-0.5,) * 3, (0.5,) * 3
    verts, tris = o.ExtractSurface(lo, hi, 32)
    v2, t2, curv = o.ExtractSurface(lo, hi, 32, curvature=True)
    assert len(tris) > 0 and verts.tobytes() == v2.tobytes() and tris.tobytes() == t2.tobytes()
    want = o._tree.query_hessian(verts, curvature=True)[3]
    assert curv.shape == (len(verts), 2) and np.array_equal(_bits(curv), _bits(want))
    sv, st, sc = o.ExtractSurface(lo, hi, 32, sparse=True, curvature=True)
    assert sv.tobytes() == verts.tobytes() and st.tobytes() == tris.tobytes() and np.array_equal(_bits(sc), _bits(curv))
    # composed with normals and project: the curvature at the final (projected) vertices, after the normals
    pv, pt, pn = o.ExtractSurface(lo, hi, 32, normals=True, project=True)
    qv, qt, qn, qc = o.ExtractSurface(lo, hi, 32, normals=True, project=True, curvature=True)
    assert qv.tobytes() == pv.tobytes() and qt.tobytes() == pt.tobytes() and qn.tobytes() == pn.tobytes()
    assert np.array_equal(_bits(qc), _bits(o._tree.query_hessian(pv, curvature=True)[3]))
    # the scalar and batched forms of the Octree
    p = (0.1, -0.2, 0.3)
    val, g, hs, cv = o.QueryHessian(p, curvature=True)
    assert isinstance(val, float) and g.shape == (3,) and hs.shape == (6,) and cv.shape == (2,) and val == o.Query(p)
    assert len(o.QueryHessian(p)) == 3
    mean, gauss = o.QueryCurvature(p)
    assert isinstance(mean, float) and np.array_equal(_bits([mean, gauss]), _bits(cv))
    vals, gs, hss = o.QueryHessian(np.array([p, (2.0, 0.0, 0.0)]), unit=True)
    assert vals[1] == DBL_MAX and np.isnan(gs[1]).all() and np.isnan(hss[1]).all() and np.array_equal(_bits(hss[0]), _bits(hs))
    means, gausses = o.QueryCurvature(np.array([p, (2.0, 0.0, 0.0)]))
    assert means.shape == (2,) and np.isnan(means[1]) and np.isnan(gausses[1]) and _bits(means)[0] == _bits(cv)[0]


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/query_hessian_caller.cpp through include/hpsdf_octree.hpp: QueryHessian scalar and batched, SurfaceCurvature -- the
    bits it prints are the Python binding's."""
    blk = _built(H, ctx, "union3_1e-7")
    rng = np.random.default_rng(283)
    pts = rng.uniform(-0.5, 0.5, (300, 3))
    pts[::37] *= 3.0
    pts[5] = np.nan
    exe = str(tmp_path / "query_hessian_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "query_hessian_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
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
    bv, bg, bh, bc = H.query_hessian_block(blk, pts, curvature=True)
    uv, ug, uh = H.query_hessian_block(blk, pts, unit=True)
    B, U, S = hexrows("B"), hexrows("U"), hexrows("S")
    assert np.array_equal(B, np.column_stack([_bits(bv), _bits(bg), _bits(bh), _bits(bc)]))
    assert np.array_equal(U, np.column_stack([_bits(uv), _bits(ug), _bits(uh)]))
    assert len(S) == 40
    for i in range(40):
        want = np.concatenate([_bits(bv)[i:i + 1], _bits(ug if i % 2 else bg)[i], _bits(bh)[i], _bits(bc)[i]])
        assert np.array_equal(S[i], want), i
    o = H.Octree()
    o.FromMemoryBlock(blk)
    verts, tris, curv = o.ExtractSurface((-0.5,) * 3, (0.5,) * 3, 24, curvature=True)
    assert rows["M"][0] == [len(verts), len(tris)] and len(verts) > 0
    assert np.array_equal(hexrows("V"), _bits(verts)) and np.array_equal(hexrows("K"), _bits(curv))
