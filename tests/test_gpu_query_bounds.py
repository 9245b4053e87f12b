"""QueryBounds on the GPU: the kernel (query_bounds.hip) and the _host entries against the device-free entries bit for bit -- every degree
class, the host-answered path, ragged last waves, the grid-stride loop, both reduction orders, subdiv 1, 2 and 4, a leaf limit, the
optional output --, the grid entry, built trees against the tree's own Query values, the per-tree constants cache, the argument checks
on the context entries, and a C++ caller of the drop-in."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hiprec as R
import surface_reference as S
from test_gpu_query_gradient import _built, _trees
from test_query_bounds_cpu import GRID_N, SUBDIVS, build_caller, grid_boxes, make_boxes
from test_surface_sparse_cpu import OFF_HI, OFF_LO

SIZES = (1, 32, 33, 63, 64, 65, 4096 + 37)
NAMES = ("lo", "hi", "status", "leaves")


def _raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def assert_rows_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_raw_bytes(g), _raw_bytes(w)), (what, name, int((_raw_bytes(g) != _raw_bytes(w)).sum()))


def _boxes_for(blk, rng):
    """make_boxes' set with rows that are no boxes of the root mixed in, at least as many as the largest size"""
    boxes = make_boxes(blk, rng, 3400, 300)
    bad = np.arange(0, len(boxes), 97)
    boxes[bad[0::4], 0] = np.nan
    boxes[bad[1::4], 3:] = boxes[bad[1::4], :3] - 1e-3
    boxes[bad[2::4], 4] = 1e9
    boxes[bad[3::4], 2] = -np.inf
    boxes = boxes[rng.permutation(len(boxes))]
    assert len(boxes) >= max(SIZES)
    return np.ascontiguousarray(boxes)


def _device_call(H, ctx, tree, boxes, n, subdiv, max_leaves, with_leaves=True):
    """hpsdf_query_bounds_device on raw device arrays -> the four arrays (leaves keeps its fill of 7 when not passed)."""
    import torch
    d_b = torch.from_numpy(np.ascontiguousarray(boxes[:n])).cuda()
    d_lo = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_hi = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_lv = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tree.query_bounds_device(d_b.data_ptr(), n, d_lo.data_ptr(), d_hi.data_ptr(), d_st.data_ptr(), d_lv.data_ptr() if with_leaves else 0,
                             subdiv=subdiv, max_leaves=max_leaves)
    ctx.synchronize()
    return d_lo.cpu().numpy(), d_hi.cpu().numpy(), d_st.cpu().numpy(), d_lv.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
def test_device_and_host_equal_block_entry_bit_for_bit(H, ctx):
    rng = np.random.default_rng(461)
    degrees, seen = set(), set()
    try:
        for name, blk in _trees(rng):
            tree = H.DeviceTree(ctx, blk)
            degrees.add(tree.info()["max_degree"])
            boxes = _boxes_for(blk, rng)
            for left in (0, 1):
                H.set_reduction_order(left)
                ctx.set_reduction_order(bool(left))
                for subdiv in SUBDIVS:
                    max_leaves = 4096 if (subdiv == 2) == bool(left) else 2     # a small limit on half of the combinations
                    what = (name, left, subdiv, max_leaves)
                    want = H.query_bounds_block(blk, boxes, subdiv, max_leaves)
                    seen |= set(int(s) for s in np.unique(want[2]))
                    for n in SIZES + (len(boxes),):
                        assert_rows_equal(tree.query_bounds(boxes[:n], subdiv, max_leaves), [w[:n] for w in want], what + (n,))
                    # the kernel for the sizes the host answers itself: raw device arrays, with and without the leaf counts
                    for n in (1, 32, 33):
                        got = _device_call(H, ctx, tree, boxes, n, subdiv, max_leaves)
                        assert_rows_equal(got, [w[:n] for w in want], what + (n, "device"))
                        bare = _device_call(H, ctx, tree, boxes, n, subdiv, max_leaves, with_leaves=False)
                        assert_rows_equal(bare[:3], [w[:n] for w in want[:3]], what + (n, "no leaf counts"))
                        assert (bare[3] == 7).all()
            tree.close()
    finally:
        ctx.set_reduction_order(None)
        H.set_reduction_order(0)
    assert {2, 3, 5, 12} <= degrees and {0, 1, 2} <= seen, (degrees, seen)


@pytest.mark.gpu
def test_grid_entry_on_the_device(H, ctx):
    import torch
    rng = np.random.default_rng(463)
    cells = GRID_N[0] * GRID_N[1] * GRID_N[2]
    shape = (GRID_N[2], GRID_N[1], GRID_N[0])
    for name, blk in _trees(rng):
        if name not in ("chain", "max3", "max5", "max12"):
            continue
        tree = H.DeviceTree(ctx, blk)
        B = R.Block(blk)                                                       # an off-centre lattice inside this tree's root
        rlo, rhi = B.root_min.astype(np.float64), B.root_max.astype(np.float64)
        OFF_LO, OFF_HI = tuple(rlo + 0.13 * (rhi - rlo)), tuple(rhi - 0.19 * (rhi - rlo))
        boxes = grid_boxes(OFF_LO, OFF_HI, GRID_N)
        for subdiv, max_leaves in ((1, 4096), (2, 3), (4, 4096)):
            what = (name, subdiv, max_leaves)
            want = H.query_bounds_grid_block(blk, OFF_LO, OFF_HI, GRID_N, subdiv, max_leaves)
            assert_rows_equal(tree.query_bounds_grid(OFF_LO, OFF_HI, GRID_N, subdiv, max_leaves), want, what)      # 455 cells: the device
            assert_rows_equal([x.reshape(shape) for x in tree.query_bounds(boxes, subdiv, max_leaves)], want, what + ("boxes",))
            d_lo = torch.full((cells,), 7.0, dtype=torch.float64, device="cuda")
            d_hi = torch.full((cells,), 7.0, dtype=torch.float64, device="cuda")
            d_st = torch.full((cells,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            tree.query_bounds_grid_device(OFF_LO, OFF_HI, GRID_N, d_lo.data_ptr(), d_hi.data_ptr(), d_st.data_ptr(), 0, subdiv, max_leaves)
            ctx.synchronize()
            got = [d_lo.cpu().numpy().reshape(shape), d_hi.cpu().numpy().reshape(shape), d_st.cpu().numpy().reshape(shape)]
            assert_rows_equal(got, want[:3], what + ("device",))
        # a lattice of a few cells is answered on the calling thread: the same bytes
        small = (3, 2, 2)
        assert_rows_equal(tree.query_bounds_grid(OFF_LO, OFF_HI, small, 2, 4096), H.query_bounds_grid_block(blk, OFF_LO, OFF_HI, small, 2, 4096),
                          (name, "12 cells"))
        tree.close()


def _cell_extrema(vals, f):
    """min and max of lattice values [f n + 1]^3 over every cell's closed range of f + 1 points per axis -> two arrays [n, n, n]"""
    lo, hi = vals, vals
    for ax in range(3):
        n = (lo.shape[ax] - 1) // f
        take = lambda a, o: np.take(a, np.arange(n) * f + o, axis=ax)
        lo = np.minimum.reduce([take(lo, o) for o in range(f + 1)])
        hi = np.maximum.reduce([take(hi, o) for o in range(f + 1)])
    return lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union3_1e-5", "union3_1e-7"])
def test_built_trees(H, ctx, case):
    """Trees Create built, root [-0.5, 0.5]^3.  4096 random boxes of edge <= 1/64 of the root: device equals block, every row is OK,
    and 32 of the tree's own Query values inside each box lie in [lo, hi].  The 32^3 cells of the root: a cell the bound decides (lo > 0
    or hi < 0) holds no value of the other sign among the 5^3 points it owns of the 4-times-finer lattice.  Both with no tolerance."""
    blk = _built(H, ctx, case)
    tree = H.DeviceTree(ctx, blk)
    rng = np.random.default_rng(467)
    c = rng.uniform(-0.5, 0.5, (4096, 3))
    e = rng.uniform(0.0, 1.0 / 64, (4096, 3))
    a, b = np.clip(c - 0.5 * e, -0.5, 0.5), np.clip(c + 0.5 * e, -0.5, 0.5)
    boxes = np.ascontiguousarray(np.concatenate([a, b], 1))
    pts = a[:, None, :] + (b - a)[:, None, :] * rng.random((4096, 32, 3))
    pts = np.minimum(np.maximum(pts, a[:, None, :]), b[:, None, :])
    q = tree.query(pts.reshape(-1, 3)).reshape(4096, 32)
    assert q.max() < 1e300
    n32 = (32, 32, 32)
    fine = tree.query(S.lattice_points((-0.5,) * 3, (0.5,) * 3, (128,) * 3)).reshape(129, 129, 129)
    vmin, vmax = _cell_extrema(fine, 4)
    for subdiv in SUBDIVS:
        got = tree.query_bounds(boxes, subdiv, 4096)
        assert_rows_equal(got, H.query_bounds_block(blk, boxes, subdiv, 4096), (case, subdiv))
        lo, hi, st, leaves = got
        assert (st == H.BOUNDS_OK).all(), (case, subdiv, np.bincount(st, minlength=4))
        assert ((lo[:, None] <= q) & (q <= hi[:, None])).all(), (case, subdiv)
        glo, ghi, gst, gleaves = tree.query_bounds_grid((-0.5,) * 3, (0.5,) * 3, n32, subdiv, 4096)
        assert (gst == H.BOUNDS_OK).all(), (case, subdiv)
        assert (glo <= vmin).all() and (vmax <= ghi).all(), (case, subdiv)
        outside, inside = glo > 0.0, ghi < 0.0
        assert (vmin[outside] > 0.0).all() and (vmax[inside] < 0.0).all(), (case, subdiv)
        straddle = float(((vmin < 0.0) & (vmax >= 0.0)).mean())
        print("%s subdiv %d: boxes decided %.4f (mean leaves %.2f); 32^3 cells decided %.4f (outside %.4f, inside %.4f; %.4f of the cells "
              "straddle the surface on the fine lattice; mean leaves %.2f)"
              % (case, subdiv, float(((lo > 0) | (hi < 0)).mean()), leaves.mean(), float((outside | inside).mean()), float(outside.mean()),
                 float(inside.mean()), straddle, gleaves.mean()))
        assert (outside | inside).mean() > 0.5, (case, subdiv)            # (the surface passes through far fewer than half of the cells)
    tree.close()


@pytest.mark.gpu
def test_a_second_call_gives_the_same_bytes(H, ctx):
    """The leaves' constants are built by the first bounds call on a tree and kept with it: a second call, and a third after another
    tree on the same context has been built, queried and destroyed in between, give the first call's bytes; so does a second handle of
    the same block (its own constants)."""
    rng = np.random.default_rng(479)
    trees = dict(_trees(rng))
    blk, other = trees["max5"], trees["max12"]
    boxes = _boxes_for(blk, rng)[:2000]
    want = H.query_bounds_block(blk, boxes, 2, 4096)
    tree = H.DeviceTree(ctx, blk)
    first = tree.query_bounds(boxes, 2, 4096)
    assert_rows_equal(first, want, "first call")
    assert_rows_equal(tree.query_bounds(boxes, 2, 4096), want, "second call")
    assert_rows_equal(tree.query_bounds(boxes[:7], 2, 4096), [w[:7] for w in want], "a call the host answers")
    t2 = H.DeviceTree(ctx, other)
    ob = _boxes_for(other, rng)[:500]
    assert_rows_equal(t2.query_bounds(ob, 1, 4096), H.query_bounds_block(other, ob, 1, 4096), "the other tree")
    t2.close()
    assert_rows_equal(tree.query_bounds(boxes, 2, 4096), want, "after another tree")
    t3 = H.DeviceTree(ctx, blk)
    assert_rows_equal(t3.query_bounds(boxes, 2, 4096), want, "a second handle")
    t3.close()
    tree.close()


@pytest.mark.gpu
def test_argument_checks_on_the_context_entries(H, ctx):
    rng = np.random.default_rng(487)
    blk = _trees(rng)[0][1]
    tree = H.DeviceTree(ctx, blk)
    boxes = _boxes_for(blk, rng)[:40].copy()
    lo, hi, st, lv = np.full(40, 7.0), np.full(40, 7.0), np.full(40, 7, np.uint8), np.full(40, 7, np.uint32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = H.lib()

    def host(tr, n, sd=1, ml=4096, b=boxes, l=lo, h=hi, s=st):
        return L.hpsdf_query_bounds_host(ctx.handle, tr, vp(b), n, sd, ml, vp(l), vp(h), vp(s), vp(lv))

    for n in (4, 40):      # the host-answered size and one that would reach the device
        for sd in (0, 3, 8):
            assert host(tree.handle, n, sd=sd) == H.ERR_INVALID_ARGUMENT
        for ml in (0, 65536):
            assert host(tree.handle, n, ml=ml) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, b=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, l=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, h=None) == H.ERR_INVALID_ARGUMENT
        assert host(tree.handle, n, s=None) == H.ERR_INVALID_ARGUMENT
        assert host(None, n) == H.ERR_INVALID_ARGUMENT
        assert (lo == 7.0).all() and (hi == 7.0).all() and (st == 7).all() and (lv == 7).all()
    assert host(tree.handle, 0, b=None, l=None, h=None, s=None) == H.OK
    assert host(tree.handle, 4, sd=4, ml=65535) == H.OK and not (st[:4] == 7).any() and (st[4:] == 7).all()
    dev = L.hpsdf_query_bounds_device
    assert dev(ctx.handle, tree.handle, None, 4, 1, 4096, None, None, None, None) == H.ERR_INVALID_ARGUMENT
    assert dev(ctx.handle, tree.handle, None, 0, 1, 4096, None, None, None, None) == H.OK
    assert dev(None, tree.handle, None, 0, 1, 4096, None, None, None, None) == H.ERR_NO_DEVICE
    lo3, hi3, n3 = (C.c_double * 3)(*OFF_LO), (C.c_double * 3)(*OFF_HI), (C.c_uint32 * 3)(3, 2, 2)
    g = [np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7, np.uint8)]
    ghost = lambda tr, l3, h3, nn, sd, ml, o: L.hpsdf_query_bounds_grid_host(ctx.handle, tr, l3, h3, nn, sd, ml, vp(o[0]), vp(o[1]), vp(o[2]), None)
    assert ghost(tree.handle, lo3, hi3, n3, 3, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, lo3, hi3, n3, 1, 0, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, None, hi3, n3, 1, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, lo3, hi3, None, 1, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, lo3, hi3, n3, 1, 4096, [None, g[1], g[2]]) == H.ERR_INVALID_ARGUMENT
    assert ghost(None, lo3, hi3, n3, 1, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, hi3, lo3, n3, 1, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert ghost(tree.handle, lo3, (C.c_double * 3)(0.2, 0.1, 0.75), n3, 1, 4096, g) == H.ERR_INVALID_ARGUMENT
    assert L.hpsdf_query_bounds_grid_device(ctx.handle, tree.handle, lo3, hi3, n3, 1, 4096, None, None, None, None) == H.ERR_INVALID_ARGUMENT
    assert all((x == 7).all() for x in g)
    assert ghost(tree.handle, lo3, hi3, n3, 1, 4096, g) == H.OK and not (g[2] == 7).any()
    tree.close()


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/bounds_caller.cpp through include/hpsdf_octree.hpp: QueryBounds batched, the scalar QueryBounds and QueryBoundsGrid --
    the bits it prints are the Python binding's."""
    from helpers import product_field
    blk = H.create_block(ctx, H.make_config(1e-5), product_field(H, "union3"), 1024)[0]
    boxes = make_boxes(blk, np.random.default_rng(491), 200, 25)
    boxes[3, 0] = np.nan
    boxes[5, 3:] = boxes[5, :3] - 0.1
    boxes[7] = (-0.5, -0.5, -0.5, 0.5, 0.5, 0.5)
    exe = build_caller(H, tmp_path)
    (tmp_path / "blk.bin").write_bytes(blk)
    (tmp_path / "boxes.bin").write_bytes(np.ascontiguousarray(boxes).tobytes())
    area = np.array(OFF_LO + OFF_HI, np.float64)
    (tmp_path / "area.bin").write_bytes(area.tobytes())
    r = subprocess.run([exe, str(tmp_path / "blk.bin"), str(tmp_path / "boxes.bin"), str(tmp_path / "area.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append([int(f[2]), int(f[3]), int(f[4], 16), int(f[5], 16)])

    def check(tag, want, count):
        got = np.array(rows[tag], np.uint64)
        bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
        assert len(got) == count, tag
        assert np.array_equal(got[:, 0], want[2][:count]) and np.array_equal(got[:, 1], want[3][:count]), tag
        assert np.array_equal(got[:, 2], bits(want[0])[:count]) and np.array_equal(got[:, 3], bits(want[1])[:count]), tag

    base, fine, two = (H.query_bounds_block(blk, boxes, sd, ml) for sd, ml in ((1, 4096), (4, 3), (2, 4096)))
    assert len(set(base[2].tolist()) | set(fine[2].tolist())) >= 3
    check("B", base, len(boxes))
    check("F", fine, len(boxes))
    mixed = [np.where(np.arange(len(boxes)) % 2 == 1, t, b) for b, t in zip(base, two)]
    check("S", mixed, 40)
    view32 = area.astype(np.float32).astype(np.float64)                      # the drop-in's area is an AlignedBox3f
    check("G", [x.ravel() for x in H.query_bounds_grid_block(blk, view32[:3], view32[3:], (5, 4, 3), 2, 4096)], 60)
    one = H.Octree()
    one.FromMemoryBlock(blk)
    lo, hi, st, leaves = one.QueryBounds(boxes[0])
    assert isinstance(lo, float) and isinstance(hi, float) and isinstance(st, int) and isinstance(leaves, int)
    assert (st, leaves) == (int(base[2][0]), int(base[3][0])) and np.float64(lo).view(np.uint64) == base[0][:1].view(np.uint64)[0]
    g = one.QueryBoundsGrid(OFF_LO, OFF_HI, 4)
    assert all(x.shape == (4, 4, 4) for x in g)
    assert_rows_equal(g, H.query_bounds_grid_block(blk, OFF_LO, OFF_HI, (4, 4, 4)), "Octree.QueryBoundsGrid")
