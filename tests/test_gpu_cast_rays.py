"""CastRays on the GPU: the kernels (cast_rays.hip) and the _host entry against the device-free entry bit for bit -- every degree class,
the few-ray kernel, the host-answered path, ragged last workgroups, both reduction orders, unit on and off, the optional outputs --,
built trees under a camera grid, and a C++ caller of the drop-in."""
import os
import subprocess

import numpy as np
import pytest

import cast_reference as CR
from conftest import ROOT
from test_cast_rays_cpu import assert_casts_equal, cast_levels, cast_rays
from test_gpu_query_gradient import _built, _trees

SIZES = (1, 32, 33, 63, 64, 65, 4096 + 37)


def _rays_for(blk, rng):
    """cast_rays' set, repeated with fresh random rays up to the largest size the kernels are run at"""
    parts = [cast_rays(blk, rng, 1400) for _ in range(3)]
    o, d, tm = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert len(o) >= max(SIZES)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tm)


def _device_call(H, ctx, tree, rays, n, iso, tol, max_iter, unit, optional=True):
    """hpsdf_cast_rays_device on raw device arrays -> the seven arrays (the optional ones keep their fill of 7 when not passed)."""
    import torch
    d_o, d_d, d_tm = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in rays)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_t = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_x = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    d_v = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_g = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    d_e = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    d_c = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    opt = [t.data_ptr() if optional else 0 for t in (d_t, d_x, d_v, d_g, d_e, d_c)]
    tree.cast_rays_device(d_o.data_ptr(), d_d.data_ptr(), d_tm.data_ptr(), n, d_st.data_ptr(), *opt, iso=iso, tol=tol, max_iter=max_iter,
                          unit=unit)
    ctx.synchronize()
    out = [t.cpu().numpy() for t in (d_st, d_t, d_x, d_v, d_g, d_e, d_c)]
    out[5], out[6] = out[5].view(np.uint16), out[6].view(np.uint16)
    return tuple(out)


@pytest.mark.gpu
def test_device_and_host_equal_block_entry_bit_for_bit(H, ctx):
    rng = np.random.default_rng(241)
    degrees, seen = set(), set()
    try:
        for name, blk in _trees(rng):
            tree = H.DeviceTree(ctx, blk)
            degrees.add(tree.info()["max_degree"])
            rays = _rays_for(blk, rng)
            _, tol = cast_levels(H, blk, rng)
            for left in (0, 1):
                H.set_reduction_order(left)
                ctx.set_reduction_order(bool(left))
                for unit in (False, True):
                    max_iter = 32 if unit == bool(left) else 2
                    what = (name, left, unit, max_iter)
                    want = H.cast_rays_block(blk, *rays, 0.0, tol, max_iter, 4096, unit)
                    seen |= set(int(s) for s in np.unique(want[0]))
                    for n in SIZES + (len(rays[0]),):
                        got = tree.cast_rays(rays[0][:n], rays[1][:n], rays[2][:n], 0.0, tol, max_iter, 4096, unit)
                        assert_casts_equal(got, [w[:n] for w in want], what + (n,))
                    # the kernels for the sizes the host answers itself: raw device arrays, with and without the optional outputs
                    for n in (1, 32, 33):
                        got = _device_call(H, ctx, tree, rays, n, 0.0, tol, max_iter, unit)
                        assert_casts_equal(got, [w[:n] for w in want], what + (n, "device"))
                        bare = _device_call(H, ctx, tree, rays, n, 0.0, tol, max_iter, unit, optional=False)
                        assert np.array_equal(bare[0], want[0][:n]), what + (n, "no optional outputs")
                        assert all((b == 7).all() for b in bare[1:])
            # a walk cut short, on the device
            want = H.cast_rays_block(blk, *rays, 0.0, tol, 32, 1)
            assert_casts_equal(tree.cast_rays(*rays, 0.0, tol, 32, 1), want, (name, "max_cells = 1"))
            seen |= set(int(s) for s in np.unique(want[0]))
            tree.close()
    finally:
        ctx.set_reduction_order(None)
        H.set_reduction_order(0)
    assert {2, 3, 5, 12} <= degrees and seen == {0, 1, 2, 3, 4}


@pytest.mark.gpu
def test_argument_checks_on_the_context_entries(H, ctx):
    import ctypes as C
    rng = np.random.default_rng(251)
    blk = _trees(rng)[0][1]
    tree = H.DeviceTree(ctx, blk)
    o, d, tm = (a[:40].copy() for a in _rays_for(blk, rng))
    st, t = np.full(40, 7, np.uint8), np.full(40, 7.0)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = H.lib()

    def host(tr, n, iso=0.0, tol=1e-9, mi=32, mc=4096, fl=0, oo=o, dd=d, tt=tm, s=st):
        return L.hpsdf_cast_rays_host(ctx.handle, tr, vp(oo), vp(dd), vp(tt), n, iso, tol, mi, mc, fl, vp(s), vp(t), None, None, None, None, None)

    for n in (4, 40):      # the host-answered size and one that would reach the device
        assert host(tree.handle, n, fl=2) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, tol=-1.0) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, tol=float("nan")) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, iso=float("inf")) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, mi=256) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, mc=0) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, mc=65536) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, s=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, oo=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, dd=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, tt=None) == H.ERR_INVALID_ARGUMENT
        assert host(None, n) == H.ERR_INVALID_ARGUMENT
        assert (st == 7).all() and (t == 7.0).all()
    assert host(tree.handle, 0, oo=None, dd=None, tt=None, s=None) == H.OK
    dev = L.hpsdf_cast_rays_device
    assert dev(ctx.handle, tree.handle, None, None, None, 4, 0.0, 1e-9, 32, 4096, 0, None, None, None, None, None, None, None) == H.ERR_INVALID_ARGUMENT
    assert dev(ctx.handle, tree.handle, None, None, None, 0, 0.0, 1e-9, 32, 4096, 0, None, None, None, None, None, None, None) == H.OK
    tree.close()


def built_rays():
    """The rays of test_built_trees for the root [-0.5, 0.5]^3: a 64 x 64 orthographic camera grid (neighbouring rows are neighbouring
    pixels; the view direction is tilted off the axes so that no ray runs inside a cell face) and 2048 random rays from a sphere
    around the root aimed at random points inside it -> (origins, directions, t_max), |d| = 1."""
    view = np.array([0.35, -0.22, -1.0])
    view /= np.linalg.norm(view)
    right = np.cross(view, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, view)
    px = (np.arange(64) + 0.5) / 64.0 - 0.5
    u, v = np.meshgrid(px, px)
    org = -2.0 * view[None, :] + 1.2 * (u.reshape(-1, 1) * right[None, :] + v.reshape(-1, 1) * up[None, :])
    cam_d = np.broadcast_to(view, org.shape)
    rng = np.random.default_rng(257)
    w = rng.normal(size=(2048, 3))
    ro = 1.5 * w / np.linalg.norm(w, axis=1, keepdims=True)
    rd = rng.uniform(-0.45, 0.45, (2048, 3)) - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    o, d = np.concatenate([org, ro]), np.concatenate([cam_d, rd])
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.full(len(o), 10.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union3_1e-5", "union3_1e-7"])
def test_built_trees(H, ctx, case):
    """Device equals block on trees Create built, under the 64 x 64 camera grid and 2048 random rays of built_rays; every HIT has
    |val| <= 1e-9; at most 5 % of the rays that cross the root end UNCONVERGED or CELL_LIMIT.  Measured beforehand with the block
    entry on the oracle's trees of the same field and targets (no device): 34 of 5952 crossing rays (0.57 %) at 1e-5 and 11 of 5952
    (0.18 %) at 1e-7, all UNCONVERGED -- sign changes on the jumps along the union's creases; 1129 and 1171 hits."""
    blk = _built(H, ctx, case)
    tree = H.DeviceTree(ctx, blk)
    rays = built_rays()
    got = tree.cast_rays(*rays, 0.0, 1e-9)
    assert_casts_equal(got, H.cast_rays_block(blk, *rays, 0.0, 1e-9), case)
    status, val, evals, cells = got[0], got[3], got[5], got[6]
    counts = np.bincount(status, minlength=5)
    crossing = int((cells >= 1).sum())
    print(case, "status counts", counts.tolist(), "rays crossing the root", crossing, "mean evaluations %.2f, mean cells %.2f"
          % (evals[cells >= 1].mean(), cells[cells >= 1].mean()))
    assert crossing >= 4096 and counts[CR.HIT] > 1000 and counts[CR.MISS] > 0 and counts[CR.INVALID] == 0
    assert (np.abs(val[status == CR.HIT]) <= 1e-9).all()
    assert counts[CR.UNCONVERGED] + counts[CR.CELL_LIMIT] <= 0.05 * crossing, counts
    tree.close()


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/cast_caller.cpp through include/hpsdf_octree.hpp: CastRays batched (world and unit gradient) and the scalar CastRay --
    the bits it prints are the Python binding's."""
    from helpers import product_field
    blk = H.create_block(ctx, H.make_config(1e-5), product_field(H, "union3"), 1024)[0]
    o, d, tm = (a[::20][:300].copy() for a in built_rays())
    o[::37] *= 3.0
    d[5] = np.nan
    tm[7] = -1.0
    tm[9] = 1.6
    exe = str(tmp_path / "cast_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "cast_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    (tmp_path / "blk.bin").write_bytes(blk)
    (tmp_path / "rays.bin").write_bytes(np.ascontiguousarray(np.concatenate([o, d, tm[:, None]], 1)).tobytes())
    r = subprocess.run([exe, str(tmp_path / "blk.bin"), str(tmp_path / "rays.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append([int(f[2]), int(f[3]), int(f[4])] + [int(x, 16) for x in f[5:]])

    def check(tag, want, count, counters=True):
        got = np.array(rows[tag], np.uint64)
        bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
        assert len(got) == count
        assert np.array_equal(got[:, 0], want[0][:count]), tag
        if counters:
            assert np.array_equal(got[:, 1], want[5][:count]) and np.array_equal(got[:, 2], want[6][:count]), tag
        assert np.array_equal(got[:, 3], bits(want[1])[:count]) and np.array_equal(got[:, 4:7], bits(want[2])[:count]), tag
        assert np.array_equal(got[:, 7], bits(want[3])[:count]) and np.array_equal(got[:, 8:11], bits(want[4])[:count]), tag

    world, unit = H.cast_rays_block(blk, o, d, tm, 0.0, 1e-9), H.cast_rays_block(blk, o, d, tm, 0.0, 1e-9, unit=True)
    assert len(set(world[0].tolist())) >= 3
    check("B", world, len(o))
    check("U", unit, len(o))
    mixed = [np.where((np.arange(len(o)) % 2 == 1).reshape((-1,) + (1,) * (w.ndim - 1)), u, w) for w, u in zip(world, unit)]
    check("S", mixed, 40, counters=False)
    one = H.Octree()
    one.FromMemoryBlock(blk)
    st, t, p, v, g, ev, ce = one.CastRays(o[0], d[0], tm[0])
    assert isinstance(st, int) and isinstance(t, float) and p.shape == (3,) and g.shape == (3,) and isinstance(ev, int) and isinstance(ce, int)
    assert (st, ev, ce) == (int(world[0][0]), int(world[5][0]), int(world[6][0]))
    assert np.array_equal(np.float64(t).view(np.uint64), world[1][:1].view(np.uint64)[0])
