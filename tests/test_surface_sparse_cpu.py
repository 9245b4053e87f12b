"""The block classification of hpsdf_extract_surface_sparse without a device: hpsdf_surface_classify_host against every lattice value
of the oracle's Query (whose values are the product's bit for bit) -- a block classed 1 or 2 must be what it says at every point of
its closed range --, the share of blocks the bound leaves to evaluate, argument errors and the new symbols."""
import os
import re

import numpy as np
import pytest

import helpers
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT_LO, ROOT_HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.3
OFF_LO, OFF_HI, OFF_N = (-0.37, -0.41, -0.29), (0.23, 0.11, 0.31), (37, 64, 23)  # off-centre, non-cubic, n not multiples of 8
BLOCK = 8


@pytest.fixture(scope="module")
def blocks(O):
    """name -> (serialised block, oracle tree)"""
    out = {}
    for name, field, target in (("union3_1e-5", O.union3_field(), 1e-5), ("union3_1e-7", O.union3_field(), 1e-7),
                                ("sphere_1e-6", O.sphere_field(SPHERE_C, SPHERE_R), 1e-6)):
        t = O.Tree.create(O.default_config(target), field, 1024, threads=8)
        out[name] = (t.to_block(), t)
    deep = helpers.deep_chain_block(np.random.default_rng(5))
    out["deep"] = (deep, O.Tree.from_block(deep))
    return out


def block_extrema(vals, n):
    """min and max of the lattice values over every block's closed point range -> two arrays [nb2, nb1, nb0]"""
    lo, hi = vals, vals
    for ax, na in ((0, n[2]), (1, n[1]), (2, n[0])):
        nb = (na + BLOCK - 1) // BLOCK
        rng = [(BLOCK * b, min(BLOCK * b + BLOCK, na) + 1) for b in range(nb)]
        lo = np.stack([np.take(lo, range(a, e), axis=ax).min(axis=ax) for a, e in rng], axis=ax)
        hi = np.stack([np.take(hi, range(a, e), axis=ax).max(axis=ax) for a, e in rng], axis=ax)
    return lo, hi


SOUND = [(name, box) for name in ("union3_1e-5", "union3_1e-7", "sphere_1e-6", "deep") for box in ("root", "off")]


@pytest.mark.parametrize("name,box", SOUND)
def test_a_culled_block_holds_no_value_on_the_other_side(H, blocks, name, box):
    block, tree = blocks[name]
    lo, hi, n = (ROOT_LO, ROOT_HI, (128, 128, 128)) if box == "root" else (OFF_LO, OFF_HI, OFF_N)
    vals = tree.query(S.lattice_points(lo, hi, n), threads=8).reshape(n[2] + 1, n[1] + 1, n[0] + 1)
    assert vals.max() < 1e300  # no point outside the root
    isos = [float(np.median(vals))] if name == "deep" else [0.0, 0.013]
    for iso in isos:
        cls = H.surface_classify_host(block, lo, hi, n, iso)
        assert cls.shape == (H.surface_block_count(n),) and cls.max() <= 2
        vmin, vmax = block_extrema(vals, n)
        vmin, vmax = vmin.ravel(), vmax.ravel()  # block index: x fastest
        assert len(vmin) == len(cls)
        bad1 = np.nonzero((cls == 1) & ~(vmin >= iso))[0]
        bad2 = np.nonzero((cls == 2) & ~(vmax < iso))[0]
        print("%s %s iso %g: classes 0/1/2 = %d/%d/%d of %d, straddling %d" % (name, box, iso, (cls == 0).sum(), (cls == 1).sum(), (cls == 2).sum(),
                                                                              len(cls), ((vmin < iso) & (vmax >= iso)).sum()))
        assert len(bad1) == 0 and len(bad2) == 0, (bad1[:8], bad2[:8])
        # a block range gives the same bytes as the whole
        assert np.array_equal(H.surface_classify_host(block, lo, hi, n, iso, first_block=5, count=40), cls[5:45])


@pytest.mark.parametrize("name", ["union3_1e-5", "union3_1e-7", "sphere_1e-6"])
def test_the_bound_culls_three_quarters_of_the_blocks_at_256(H, blocks, name):
    cls = H.surface_classify_host(blocks[name][0], ROOT_LO, ROOT_HI, (256, 256, 256), 0.0)
    share = float((cls == 0).mean())
    print("%s: class-0 share at n = 256: %.4f" % (name, share))
    assert (cls == 1).any() and (cls == 2).any()
    assert share <= 0.25


def test_argument_errors(H, blocks):
    block = blocks["sphere_1e-6"][0]
    bad = [
        (ROOT_LO, ROOT_HI, (8, 0, 8), 0.0, {}, "axis y"),
        ((0.1, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, {}, "axis x"),
        ((0.2, -0.5, -0.5), (0.1, 0.5, 0.5), (8, 8, 8), 0.0, {}, "axis x"),
        (ROOT_LO, ROOT_HI, (1 << 20, 1 << 20, 1), 0.0, {"count": 1}, "2^40"),
        (ROOT_LO, ROOT_HI, ((1 << 20) + 1, 8, 8), 0.0, {"count": 1}, "2^20"),
        (ROOT_LO, ROOT_HI, (16, 16, 16), 0.0, {"first_block": 7, "count": 2}, "past"),
        (ROOT_LO, ROOT_HI, (16, 16, 16), 0.0, {"first_block": 9, "count": 0}, "past"),
        (ROOT_LO, ROOT_HI, (16, 16, 16), float("nan"), {}, "iso"),
        (ROOT_LO, (0.5, 0.5, 0.75), (16, 16, 16), 0.0, {}, "axis z"),
    ]
    for lo, hi, n, iso, kw, msg in bad:
        with pytest.raises(H.HpsdfError) as ei:
            H.surface_classify_host(block, lo, hi, n, iso, **kw)
        assert ei.value.status == 1 and msg in str(ei.value), (lo, hi, n, str(ei.value))
    with pytest.raises(H.HpsdfError):
        H.surface_classify_host(block[:-8], ROOT_LO, ROOT_HI, (16, 16, 16))
    assert len(H.surface_classify_host(block, ROOT_LO, ROOT_HI, (16, 16, 16), first_block=8, count=0)) == 0
    assert len(H.surface_classify_host(block, ROOT_LO, ROOT_HI, (16, 16, 16))) == 8
    # the largest lattice the contract allows is accepted (one block of it is classified)
    assert len(H.surface_classify_host(block, ROOT_LO, ROOT_HI, (10000, 10000, 10000), first_block=12345, count=1)) == 1


def test_new_symbols_are_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_extract_surface_sparse", "hpsdf_surface_classify_host", "hpsdf_surface_classify_device"}
    assert new <= declared and declared == set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == 4 == H.ABI_VERSION
    assert int(re.search(r"#define HPSDF_SURFACE_BLOCK (\d+)", hdr).group(1)) == H.SURFACE_BLOCK == BLOCK
    import ctypes as C
    assert C.sizeof(H.SurfaceSparseStats) == 96
