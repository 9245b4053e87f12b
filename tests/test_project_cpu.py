"""ProjectToSurface without a device: hpsdf_project_block (the statements of the kernels on the calling thread) against the numpy
restatement of tests/project_reference.py bit for bit, the invariants of every row, the optional outputs, the in-place call, the
argument checks, a built sphere against the fit's own error, and the acceptance rule for mesh vertices."""
import ctypes as C

import numpy as np
import pytest

import hiprec as R
import project_reference as P
from helpers import edge_points, synthetic_block
from test_hiprec_cpu import ROOTS
from test_query_gradient_cpu import gradient_blocks

DBL_MAX = np.finfo(np.float64).max
SEED = 101


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def project_trees(rng):
    """gradient_blocks (every degree 0..12, depths to 10, three roots) and trees whose largest degree is 2 (every leaf in the top
    table), 3, 5 and 12: the degree classes the kernels are instantiated for."""
    out = gradient_blocks(rng)
    out.append(("max2-top", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)))
    out.append(("max3", synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)))
    out.append(("max5", synthetic_block(rng, [5, 4, 3, 2, 1, 0, 5, 4], 2, *ROOTS["cube"])))
    out.append(("max12", synthetic_block(rng, [12, 7, 3, 2, 9, 0, 5, 6], 2)))
    return out


def project_points(blk, rng, n_in_leaves=2048):
    B = R.Block(blk)
    lo, hi = B.root_min.astype(np.float64), B.root_max.astype(np.float64)
    bad = lo + (hi - lo) * rng.uniform(0.0, 1.0, (64, 3))
    bad[:16, 0] = hi[0] + (hi[0] - lo[0]) * rng.uniform(0.01, 3.0, 16)
    bad[16:32, 1] = lo[1] - (hi[1] - lo[1]) * rng.uniform(0.01, 3.0, 16)
    bad[32:40] = np.nan
    bad[40:48, 2] = np.nan
    bad[48:56, 0] = np.inf
    bad[56:64] = -np.inf
    pts = np.concatenate([R.points_in_leaves(B, rng, n_in_leaves), B.from_unit(edge_points(rng)), bad])
    return pts[rng.permutation(len(pts))]


def levels(H, blk, pts):
    """(iso values, tol) of the parity tests: iso 0 and the median field value; tol = 1e-9 max|f| over the rows inside the root."""
    f = H.query_gradient_block(blk, pts)[0]
    f = f[f != DBL_MAX]
    return (0.0, float(np.median(f))), 1e-9 * float(np.abs(f).max())


def assert_rows_equal(got, want, what):
    for name, g, w in zip(("xyz", "val", "grad"), got[:3], want[:3]):
        assert np.array_equal(_bits(g), _bits(w)), (what, name, int((_bits(g) != _bits(w)).sum()))
    assert got[3].dtype == np.uint8 and got[4].dtype == np.uint8
    assert np.array_equal(got[3], want[3]), (what, "iters")
    assert np.array_equal(got[4], want[4]), (what, "status")


def _raw(H, block, pts, n, iso, tol, max_iter, flags, out_xyz, val=None, grad=None, iters=None, status=None):
    buf = bytes(block)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return H.lib().hpsdf_project_block(buf, len(buf), vp(pts), n, iso, tol, max_iter, flags, vp(out_xyz), vp(val), vp(grad), vp(iters), vp(status))


# ------------------------------------------------------------------------------------------------------------ parity and invariants
def test_block_entry_equals_the_restatement_bit_for_bit(H):
    rng = np.random.default_rng(SEED)
    before = H.reduction_order()
    seen = set()
    try:
        for name, blk in project_trees(rng):
            pts = project_points(blk, rng)
            isos, tol = levels(H, blk, pts)
            for left in (0, 1):
                H.set_reduction_order(left)
                for unit in (False, True):
                    for iso in isos:
                        for max_iter in (0, 1, 8):
                            what = (name, left, unit, iso, max_iter)
                            want = P.project_reference(H, blk, pts, iso, tol, max_iter, unit, left)
                            got = H.project_block(blk, pts, iso, tol, max_iter, unit)
                            assert_rows_equal(got, want, what)
                            seen |= set(int(s) for s in np.unique(want[4]))
                            _check_invariants(H, blk, got, iso, tol, max_iter, unit, left, what)
    finally:
        H.set_reduction_order(before)
    assert seen == {P.CONVERGED, P.ITER_LIMIT, P.LEFT_ROOT, P.FLAT}, seen


def _check_invariants(H, blk, rows, iso, tol, max_iter, unit, left, what):
    x, val, grad, iters, status = rows
    qv, qg = H.query_gradient_block(blk, x, unit=unit)
    assert np.array_equal(_bits(val), _bits(qv)) and np.array_equal(_bits(grad), _bits(qg)), what
    with np.errstate(invalid="ignore"):
        assert np.array_equal(status == P.CONVERGED, (val != DBL_MAX) & (np.abs(val - iso) <= tol)), what
    assert (iters[status == P.ITER_LIMIT] == max_iter).all() and (iters <= max_iter).all(), what
    assert np.array_equal(status == P.LEFT_ROOT, val == DBL_MAX), what
    assert np.isnan(grad[status == P.LEFT_ROOT]).all(), what
    g = H.query_gradient_block(blk, x[status == P.FLAT])[1]
    z = P.sum3(g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2], left)
    assert not (z > 0).any(), what


def test_every_status_is_exercised_per_kind_of_tree(H):
    """What the seed was chosen for, from the restatement alone: degree-0 leaves give FLAT, points near the root faces LEFT_ROOT, and
    the degree-3 and degree-12 trees a few ITER_LIMIT at max_iter = 8."""
    rng = np.random.default_rng(SEED)
    trees = dict(project_trees(rng))
    for name in ("max3", "max12"):
        rng = np.random.default_rng(SEED + 1)
        pts = project_points(trees[name], rng)
        _, tol = levels(H, trees[name], pts)
        status = P.project_reference(H, trees[name], pts, 0.0, tol, 8)[4]
        assert set(np.unique(status)) == {0, 1, 2, 3}, (name, np.bincount(status))


# ------------------------------------------------------------------------------------------------------------ optional outputs, in place
def test_null_optional_outputs_and_in_place(H):
    rng = np.random.default_rng(103)
    blk = synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)
    pts = project_points(blk, rng, 256)
    n = len(pts)
    _, tol = levels(H, blk, pts)
    full = H.project_block(blk, pts, 0.0, tol, 8, True)
    fresh = lambda: (np.full((n, 3), 7.0), np.full(n, 7.0), np.full((n, 3), 7.0), np.full(n, 7, np.uint8), np.full(n, 7, np.uint8))
    for keep in range(1, 5):          # every optional output alone, the others NULL
        bufs = fresh()
        args = [bufs[i] if i == keep else None for i in range(1, 5)]
        assert _raw(H, blk, pts, n, 0.0, tol, 8, 1, bufs[0], *args) == H.OK
        assert np.array_equal(_bits(bufs[0]), _bits(full[0]))
        assert np.array_equal(bufs[keep].view(np.uint8), np.ascontiguousarray(full[keep]).view(np.uint8)), keep
    bufs = fresh()
    assert _raw(H, blk, pts, n, 0.0, tol, 8, 1, bufs[0]) == H.OK and np.array_equal(_bits(bufs[0]), _bits(full[0]))
    # out_xyz aliasing the input
    inout = pts.copy()
    bufs = fresh()
    assert _raw(H, blk, inout, n, 0.0, tol, 8, 1, inout, *bufs[1:]) == H.OK
    assert_rows_equal((inout,) + bufs[1:], full, "in place")


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(H):
    rng = np.random.default_rng(107)
    blk = synthetic_block(rng, list(range(8)), 1)
    pts = rng.uniform(-0.4, 0.4, (4, 3))
    bufs = (np.full((4, 3), 7.0), np.full(4, 7.0), np.full((4, 3), 7.0), np.full(4, 7, np.uint8), np.full(4, 7, np.uint8))
    untouched = lambda: all((b == 7).all() for b in bufs)
    assert _raw(H, blk, pts, 0, 0.0, 1e-9, 16, 0, *bufs) == H.OK and untouched()
    assert _raw(H, blk, None, 0, 0.0, 1e-9, 16, 1, None) == H.OK
    bad = [dict(flags=2), dict(flags=0x80000001), dict(tol=-1e-300), dict(tol=float("nan")), dict(iso=float("inf")),
           dict(iso=float("-inf")), dict(iso=float("nan")), dict(max_iter=256), dict(max_iter=0xFFFFFFFF)]
    for kw in bad:
        a = dict(iso=0.0, tol=1e-9, max_iter=16, flags=0)
        a.update(kw)
        assert _raw(H, blk, pts, 4, a["iso"], a["tol"], a["max_iter"], a["flags"], *bufs) == H.ERR_INVALID_ARGUMENT, kw
        assert H.lib().hpsdf_last_error() and untouched(), kw
    assert _raw(H, blk, pts, 4, 0.0, 1e-9, 16, 4, *bufs) == H.ERR_INVALID_ARGUMENT and b"flag" in H.lib().hpsdf_last_error()
    assert _raw(H, blk, pts, 4, 0.0, 1e-9, 16, 0, None, *bufs[1:]) == H.ERR_INVALID_ARGUMENT and untouched()       # NULL out_xyz
    assert _raw(H, blk, None, 4, 0.0, 1e-9, 16, 0, *bufs) == H.ERR_INVALID_ARGUMENT and untouched()
    assert _raw(H, blk, pts, 4, 0.0, 0.0, 255, 1, *bufs) == H.OK and not untouched()                             # the limits themselves pass
    bufs = (np.full((4, 3), 7.0), np.full(4, 7.0), np.full((4, 3), 7.0), np.full(4, 7, np.uint8), np.full(4, 7, np.uint8))
    for cut in (blk[:-1], blk[:100], blk[:8], b""):
        assert _raw(H, cut, pts, 4, 0.0, 1e-9, 16, 0, *bufs) == H.ERR_BAD_BLOCK and H.lib().hpsdf_last_error() and untouched()
    with pytest.raises(H.HpsdfError):
        H.project_block(blk[:-8], pts)
    with pytest.raises(H.HpsdfError) as ei:
        H.project_block(blk, pts, max_iter=300)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT


def test_new_symbols_are_declared_bound_and_exported(H):
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_project_device", "hpsdf_project_host", "hpsdf_project_block", "hpsdf_surface_project_vertices"}
    assert new <= declared and new <= set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    assert int(re.search(r"#define HPSDF_PROJECT_UNIT (\d+)u", hdr).group(1)) == H.PROJECT_UNIT
    m = re.search(r"enum \{ HPSDF_PROJECT_CONVERGED = (\d), HPSDF_PROJECT_ITER_LIMIT = (\d), HPSDF_PROJECT_LEFT_ROOT = (\d), HPSDF_PROJECT_FLAT = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.PROJECT_CONVERGED, H.PROJECT_ITER_LIMIT, H.PROJECT_LEFT_ROOT, H.PROJECT_FLAT) == (0, 1, 2, 3)
    assert H.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------------------ a built sphere
def test_sphere_projection_reaches_the_fits_own_error(H, O):
    """The oracle's sphere tree at 1e-8 (centre (0.25, 0, 0), radius 0.5), 4000 points uniform in [-0.49, 0.49]^3, tol 1e-9, 16 steps:
    every row converges or leaves the root, none runs into the iteration limit; converged rows have |value| <= tol and lie within
    2 E + tol of the true sphere, E being the fit's own error max |Query - true| over 20 000 random points inside the root as the
    ORACLE's Tree.query evaluates it (the factor 2: E is a sampled maximum).  Measured when this was written: E = 2.9e-4 (taken where
    the fit is coarsest, near the sphere's centre, far from the surface), the largest distance 3.7e-6, 3821 rows converged and 179
    left the root, at most 3 steps a converged row."""
    tree = O.Tree.create(O.default_config(1e-8), O.sphere_field(), 1024)
    blk = tree.to_block()
    centre, radius, tol = np.array([0.25, 0.0, 0.0]), 0.5, 1e-9
    rng = np.random.default_rng(109)
    probe = rng.uniform(-0.5, 0.5, (20000, 3))
    E = float(np.abs(tree.query(probe) - (np.linalg.norm(probe - centre, axis=1) - radius)).max())
    pts = rng.uniform(-0.49, 0.49, (4000, 3))
    x, val, grad, iters, status = H.project_block(blk, pts, 0.0, tol, 16)
    conv = status == P.CONVERGED
    dist = np.abs(np.linalg.norm(x[conv] - centre, axis=1) - radius)
    print("E %.3g, status counts %s, max |val| %.3g, max distance %.3g, max iters of converged rows %d"
          % (E, np.bincount(status, minlength=4).tolist(), np.abs(val[conv]).max(), dist.max(), iters[conv].max()))
    assert np.isin(status, (P.CONVERGED, P.LEFT_ROOT)).all() and not (status == P.ITER_LIMIT).any()
    assert conv.sum() > 2000
    assert (np.abs(val[conv]) <= tol).all()
    assert (dist <= 2 * E + tol).all(), (dist.max(), E)
    assert_rows_equal((x, val, grad, iters, status), P.project_reference(H, blk, pts, 0.0, tol, 16), "sphere")


# ------------------------------------------------------------------------------------------------------------ the vertex rule
def test_vertex_acceptance_rule():
    h = (0.25, 0.5, 1.0)
    v = np.zeros((8, 3))
    p = np.array([[0.125, 0.25, 0.5],            # exactly half a cube on every axis: accepted
                  [np.nextafter(0.125, 1.0), 0.0, 0.0],   # one ulp past it on x: stays
                  [0.0, -0.25, 0.0],             # the lower side, on the limit: accepted
                  [0.0, 0.0, -0.5000001],        # past it on z: stays
                  [0.01, 0.01, 0.01],            # converged ... but status 1: stays
                  [0.01, 0.01, 0.01],            # status 2
                  [np.nan, 0.0, 0.0],            # a NaN never passes the comparison
                  [0.0, 0.0, 0.0]])              # projection equal to the vertex: counted as replaced
    status = np.array([0, 0, 0, 0, 1, 2, 0, 0], np.uint8)
    out, moved = P.accept_vertices(v, p, status, h)
    assert moved == 3
    assert np.array_equal(out[[0, 2, 7]], p[[0, 2, 7]]) and (out[[1, 3, 4, 5, 6]] == 0).all()
    for s in (1, 2, 3):
        assert P.accept_vertices(v, p, np.full(8, s, np.uint8), h)[1] == 0
