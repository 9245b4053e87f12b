"""Simplify on the device (include/hpsdf.h, "Simplify"; csrc/simplify.hip): hpsdf_simplify returns the bytes and the stats of
hpsdf_simplify_block -- which tests/test_simplify_cpu.py holds against the long-double reference -- on every shape at which the kernels
take another path: both degree classes, the largest LDS cube, mixed degrees, the 83-row degree 6, ten levels, trees the product built."""
import numpy as np
import pytest

import hiprec as HR
import simplify_reference as SR
from helpers import deep_chain_block, edge_points, product_field, query_points
from hiprec import COUNT, INTERIOR

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(H, ctx, blk, rms, what, **kw):
    want, wst = H.simplify_block(blk, rms, **kw)
    got, gst = H.simplify(ctx, blk, rms, **kw)
    assert got == want, (what, rms, kw, gst, wst)
    assert gst == wst, (what, rms, kw, gst, wst)
    return got, gst


def _random_depth2(rng, degrees):
    return SR.make_depth2_block([rng.standard_normal(int(COUNT[d])) for d in degrees], degrees)


@pytest.fixture(scope="module")
def built(H, ctx):
    return {(name, target): H.create_block(ctx, H.make_config(target), product_field(H, name), 1024)[0]
            for name, target in (("sphere", 1e-4), ("union3", 1e-5), ("union3", 1e-7))}


# ------------------------------------------------------------------------------------------------------------ 1
def test_exact_merge_block(H, ctx):
    blk = SR.exact_merge_block(np.random.default_rng(41), [4, 4, 4, 1, 2, 4, 2, 1], 4)[0]
    out, st = _same(H, ctx, blk, 1e-9, "exact merge")
    assert st["merges"] == 8 and st["nodes_out"] == 9
    for kw in ({"truncate": False}, {"merge": False}, {"flags": 0}):
        _same(H, ctx, blk, 1e-9, "exact merge", **kw)
    assert H.simplify(ctx, blk, 0.0)[0] == blk


def test_deep_chain(H, ctx):
    blk = deep_chain_block(np.random.default_rng(5), 10, (2, 3, 1, 0, 4, 3, 2, 5))
    # random rows of unit size: a cell at depth 9 has volume 8^-9, so nothing merges until rms^2 8^-9 reaches the rows' energy (~1e2);
    # the chain merges from the bottom, one candidate a level, nine levels
    merges = [_same(H, ctx, blk, rms, "deep chain")[1]["merges"] for rms in (1e-3, 1e3, 1e8)]
    assert merges[0] == 0 and merges[2] == 9
    st = _same(H, ctx, blk, 1e8, "deep chain", truncate=False)[1]
    assert st["merges"] == 9 and st["levels"] == 9 and st["nodes_out"] == 9


def test_degree_12(H, ctx):
    """64 leaves of degree 12: the largest cube the workgroup class holds in LDS."""
    rng = np.random.default_rng(7)
    out, st = _same(H, ctx, _random_depth2(rng, [12] * 64), 1e-3, "degree 12, random rows")
    assert st["merges"] == 0 and st["nodes_out"] == 73
    blk = SR.exact_merge_block(rng, [12] * 8, 12)[0]
    out, st = _same(H, ctx, blk, 1e-9, "degree 12, restricted parents")
    assert st["merges"] == 8 and st["nodes_out"] == 9 and (HR.Block(out).degree[1:] == 12).all()


def test_degree_classes(H, ctx):
    """Every degree as the largest of a candidate (5 | 6 is the border between the wave class and the workgroup class; 6 stores 83 of its
    84 entries), with children of lower degrees beside it, accepted (a huge rms) and rejected."""
    rng = np.random.default_rng(11)
    degrees = []
    for p in range(8):
        top = [0, 3, 5, 6, 7, 9, 11, 12][p]
        degrees += [top] + [int(d) for d in rng.integers(0, top + 1, 7)]
    blk = _random_depth2(rng, degrees)
    out, st = _same(H, ctx, blk, 1e6, "mixed degrees, accepted")
    assert st["merges"] == 8
    _same(H, ctx, blk, 1e6, "mixed degrees, accepted", truncate=False)
    assert _same(H, ctx, blk, 1e-6, "mixed degrees, rejected")[1]["merges"] == 0
    for child in (5, 6, 7):
        blk = SR.exact_merge_block(rng, [child, child, 2, child, 0, child, 1, child], child)[0]
        assert _same(H, ctx, blk, 1e-9, "restricted parents at degree %d" % child)[1]["merges"] == 8


def test_built_trees(H, ctx, built):
    for name, target in (("sphere", 1e-4), ("union3", 1e-5)):
        for rms in (1e-4, 1e-3, 1e-2):
            out, st = _same(H, ctx, built[name, target], rms, (name, target))
            print(name, target, rms, st)
    out, st = _same(H, ctx, built["union3", 1e-7], 1e-3, ("union3", 1e-7))
    print("union3", 1e-7, 1e-3, st)
    assert st["levels"] > 1 and st["merges"] > 0 and st["truncations"] > 0
    src = HR.Block(built["union3", 1e-7])
    assert len(set(src.degree[src.degree != INTERIOR])) > 1


# ------------------------------------------------------------------------------------------------------------ 2
def test_octree_simplify(H, O, built):
    blk = built["union3", 1e-5]
    o = H.Octree()
    o.FromMemoryBlock(blk)
    small, st = o.Simplify(1e-3, stats=True)
    assert small is not o and small.ctx is o.ctx and o.ToMemoryBlock() == blk            # the source is unchanged
    out = small.ToMemoryBlock()
    assert out == H.simplify_block(blk, 1e-3)[0] and st["nodes_out"] < st["nodes_in"]
    rng = np.random.default_rng(47)
    pts = np.concatenate([query_points(O, (-0.5,) * 3, (0.5,) * 3, 10000), HR.Block(out).from_unit(edge_points(rng))])
    assert np.array_equal(_bits(small.Query(pts)), _bits(H.query_gradient_block(out, pts)[0]))
    assert np.array_equal(_bits(o.Query(pts)), _bits(H.query_gradient_block(blk, pts)[0]))
    merged = o.Simplify(1e-3, truncate=False)
    assert merged.ToMemoryBlock() == H.simplify_block(blk, 1e-3, truncate=False)[0]
    with pytest.raises(H.HpsdfError) as ei:
        o.Simplify(float("nan"))
    assert ei.value.status == H.ERR_INVALID_ARGUMENT
    again = H.Octree()
    again.FromMemoryBlock(out)                                                           # the result is a block like any other
    assert np.array_equal(_bits(again.Query(pts)), _bits(small.Query(pts)))


# ------------------------------------------------------------------------------------------------------------ 3
def test_cxx_caller(H, ctx, built, tmp_path):
    """tests/native/simplify_caller.cpp through include/hpsdf_octree.hpp against the device path: the same bytes and stats."""
    from test_simplify_cpu import build_caller, run_caller
    exe = build_caller(H, tmp_path)
    blk = built["union3", 1e-5]
    for rms, flags in ((1e-3, 3), (1e-2, 1)):
        got, stats = run_caller(exe, tmp_path, blk, rms, flags, "device")
        want, st = H.simplify(ctx, blk, rms, flags=flags)
        assert got == want and stats == st
        assert got == H.simplify_block(blk, rms, flags=flags)[0]
