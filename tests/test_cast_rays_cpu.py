"""CastRays without a device: hpsdf_cast_rays_block (the statements of the kernels on the calling thread) against the numpy restatement
of tests/cast_reference.py bit for bit, the invariants of every row checked without the restatement, every status, the optional
outputs, the argument checks, and a sphere built by the oracle against the analytic ray-sphere parameter."""
import ctypes as C

import numpy as np
import pytest

import cast_reference as CR
import hiprec as R
from test_project_cpu import project_trees

DBL_MAX = np.finfo(np.float64).max
SEED = 131
OUT_NAMES = ("status", "t", "xyz", "val", "grad", "evals", "cells")


def _raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def assert_casts_equal(got, want, what):
    for name, g, w in zip(OUT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype)
        bad = np.nonzero((_raw_bytes(g) != _raw_bytes(w)).any(1))[0]
        assert len(bad) == 0, (what, name, len(bad), bad[:8].tolist())


def cast_rays(blk, rng, n_random=160):
    """(origins, directions, t_max) for a block: random origins inside and outside the root aimed at random points inside (d not
    normalised); axis-parallel rays (one or two zero direction components); rays lying in cell mid-planes and along root faces (a
    coordinate held on a dyadic plane by a zero direction component); rays that miss the root; NaN and inf rows, a zero direction,
    negative and NaN t_max.  t_max is infinite, ample, or short enough to end inside the root."""
    B = R.Block(blk)
    lo, hi = B.root_min.astype(np.float64), B.root_max.astype(np.float64)
    ext = hi - lo
    o, d = [], []
    # aimed
    tgt = lo + ext * rng.uniform(0.0, 1.0, (n_random, 3))
    org = lo + ext * rng.uniform(-1.0, 2.0, (n_random, 3))
    org[::3] = lo + ext * rng.uniform(0.0, 1.0, (len(org[::3]), 3))
    o.append(org), d.append((tgt - org) * rng.uniform(0.3, 3.0, (n_random, 1)))
    # axis-parallel: one moving axis, then two
    for moving in (1, 2):
        m = 36
        org = lo + ext * rng.uniform(0.0, 1.0, (m, 3))
        dd = np.zeros((m, 3))
        for i in range(m):
            axes = rng.permutation(3)[:moving]
            sgn = rng.choice([-1.0, 1.0], moving)
            dd[i, axes] = sgn * rng.uniform(0.2, 2.0, moving) * ext[axes]
            if i % 2:
                org[i, axes[0]] = (lo - ext)[axes[0]] if sgn[0] > 0 else (hi + ext)[axes[0]]
        o.append(org), d.append(dd)
    # in cell mid-planes and along root faces: unit coordinate on a dyadic plane, zero direction component there
    planes = np.array([0.0, 0.25, -0.25, 0.125, -0.375, 0.5, -0.5])
    m = 42
    q = rng.uniform(-0.5, 0.5, (m, 3))
    dq = rng.uniform(-1.0, 1.0, (m, 3))
    for i in range(m):
        a = i % 3
        q[i, a] = planes[i % len(planes)]
        dq[i, a] = 0.0
        if i % 4 == 0:          # two coordinates on planes: the ray runs along a cell edge
            b = (a + 1) % 3
            q[i, b] = planes[(i // 3) % len(planes)]
            dq[i, b] = 0.0
        if i % 5 == 0:          # start outside, behind the root
            c = (a + 2) % 3
            q[i, c] = -1.5 if dq[i, c] > 0 else 1.5
    o.append(B.from_unit(q)), d.append(dq * ext)
    # misses: aimed away from the root, or parallel to it beside it
    m = 24
    org = lo + ext * rng.uniform(1.2, 2.5, (m, 3))
    dd = rng.uniform(0.1, 1.0, (m, 3)) * ext
    dd[::2, 0] = 0.0
    dd[1::4] *= -1.0                                             # (these point at the root's corner region: some hit the root)
    o.append(org), d.append(dd)
    # rows that are not rays
    bad_o = lo + ext * rng.uniform(0.0, 1.0, (16, 3))
    bad_d = rng.uniform(-1.0, 1.0, (16, 3))
    bad_o[0] = np.nan
    bad_o[1, 2] = np.nan
    bad_o[2, 0] = np.inf
    bad_o[3] = -np.inf
    bad_d[4] = np.nan
    bad_d[5, 1] = np.nan
    bad_d[6, 2] = np.inf
    bad_d[7] = -np.inf
    bad_d[8] = 0.0
    bad_d[9] = -0.0
    o.append(bad_o), d.append(bad_d)
    o, d = np.concatenate(o), np.concatenate(d)
    n = len(o)
    t_max = np.full(n, np.inf)
    t_max[1::3] = 50.0
    t_max[2::3] = rng.uniform(0.0, 1.5, len(t_max[2::3]))
    t_max[n - 6] = -1.0
    t_max[n - 5] = np.nan
    t_max[n - 4] = -np.inf
    t_max[n - 3] = 0.0
    perm = rng.permutation(n)
    return o[perm], d[perm], t_max[perm]


def cast_levels(H, blk, rng):
    """(iso values, tol): iso 0 and the median field value, tol = 1e-9 max|f|, over 2048 points in the block's leaves."""
    f = H.query_gradient_block(blk, R.points_in_leaves(blk, rng, 2048))[0]
    return (0.0, float(np.median(f))), 1e-9 * float(np.abs(f).max())


def check_invariants(H, blk, rays, rows, iso, tol, max_iter, max_cells, unit, what):
    """What a row must satisfy whatever the walk did, from the header's output section alone."""
    o, d, t_max = rays
    status, t, x, val, grad, evals, cells = rows
    fin = np.isfinite(t)
    assert np.array_equal(fin, np.isin(status, (CR.HIT, CR.UNCONVERGED))), what
    assert np.isnan(t[np.isin(status, (CR.MISS, CR.INVALID, CR.CELL_LIMIT))]).all(), what
    with np.errstate(all="ignore"):
        want_x = np.full_like(x, np.nan)
        for a in range(3):
            m = t[fin] * d[fin, a]
            want_x[fin, a] = o[fin, a] + m
    assert np.array_equal(_raw_bytes(x), _raw_bytes(want_x)), what
    qv, qg = H.query_gradient_block(blk, x, unit=unit)
    assert np.array_equal(_raw_bytes(val), _raw_bytes(qv)) and np.array_equal(_raw_bytes(grad), _raw_bytes(qg)), what
    assert np.array_equal(status[fin] == CR.HIT, np.abs(val[fin] - iso) <= tol), what
    assert (t[fin] >= 0).all() and (t[fin] <= t_max[fin]).all(), what
    assert (cells <= max_cells).all() and (cells[status == CR.CELL_LIMIT] == max_cells).all(), what
    # an evaluation for the first sample, at most max(1, p) <= 12 per leaf, at most max_iter in the refinement
    assert (evals.astype(np.int64) <= 1 + 12 * cells.astype(np.int64) + max_iter).all(), what
    assert (evals[status == CR.INVALID] == 0).all() and (evals[fin] >= 1).all(), what


# ------------------------------------------------------------------------------------------------------------ parity and invariants
def test_block_entry_equals_the_restatement_bit_for_bit(H):
    rng = np.random.default_rng(SEED)
    before = H.reduction_order()
    seen, classes = set(), set()
    try:
        for name, blk in project_trees(rng):
            rays = cast_rays(blk, rng)
            isos, tol = cast_levels(H, blk, rng)
            classes.add(int(R.Block(blk).degree[R.Block(blk).leaves()].max()))
            for left in (0, 1):
                H.set_reduction_order(left)
                for iso in isos:
                    for max_iter in (0, 2, 32):
                        unit = bool((left + max_iter) % 4 == 0)
                        what = (name, left, iso, max_iter, unit)
                        want = CR.cast_reference(H, blk, *rays, iso, tol, max_iter, 4096, unit, left)
                        got = H.cast_rays_block(blk, *rays, iso, tol, max_iter, 4096, unit)
                        assert_casts_equal(got, want, what)
                        check_invariants(H, blk, rays, got, iso, tol, max_iter, 4096, unit, what)
                        seen |= set(int(s) for s in np.unique(got[0]))
                # a walk cut short: one leaf, then a few
                for max_cells in (1, 3):
                    what = (name, left, "max_cells", max_cells)
                    want = CR.cast_reference(H, blk, *rays, isos[0], tol, 32, max_cells, False, left)
                    got = H.cast_rays_block(blk, *rays, isos[0], tol, 32, max_cells)
                    assert_casts_equal(got, want, what)
                    check_invariants(H, blk, rays, got, isos[0], tol, 32, max_cells, False, what)
                    assert max_cells > 1 or (got[0] == CR.CELL_LIMIT).any(), what
                    seen |= set(int(s) for s in np.unique(got[0]))
    finally:
        H.set_reduction_order(before)
    assert seen == {CR.HIT, CR.MISS, CR.UNCONVERGED, CR.CELL_LIMIT, CR.INVALID}, seen
    assert {2, 3, 5, 12} <= classes, classes


def test_every_status_occurs_on_one_tree_and_the_walk_crosses_leaves(H):
    """The random-coefficient trees jump across every cell face, so UNCONVERGED is plentiful; the deep chain makes rays cross several
    leaves; max_cells = 1 cuts every ray that leaves its first leaf."""
    rng = np.random.default_rng(SEED + 1)
    trees = dict(project_trees(rng))
    blk = trees["chain"]
    rays = cast_rays(blk, rng)
    _, tol = cast_levels(H, blk, rng)
    full = H.cast_rays_block(blk, *rays, 0.0, tol)
    status, evals, cells = full[0], full[5], full[6]
    counts = np.bincount(status, minlength=5)
    print("chain: status counts", counts.tolist(), "largest cells", int(cells.max()), "largest evals", int(evals.max()))
    assert counts[CR.HIT] and counts[CR.MISS] and counts[CR.UNCONVERGED] and counts[CR.INVALID] and not counts[CR.CELL_LIMIT]
    assert cells.max() >= 4
    one = H.cast_rays_block(blk, *rays, 0.0, tol, max_cells=1)
    assert (one[0] == CR.CELL_LIMIT).any() and (one[6] <= 1).all()
    # a ray that stopped without leaving its first leaf is the same row under either limit
    same = one[0] != CR.CELL_LIMIT
    assert same.any() and not same.all()
    assert_casts_equal([a[same] for a in one], [a[same] for a in full], "max_cells = 1")


# ------------------------------------------------------------------------------------------------------------ optional outputs
def _raw(H, block, rays, n, iso, tol, max_iter, max_cells, flags, status, t=None, xyz=None, val=None, grad=None, evals=None, cells=None):
    buf = bytes(block)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    o, d, tm = rays
    return H.lib().hpsdf_cast_rays_block(buf, len(buf), vp(o), vp(d), vp(tm), n, iso, tol, max_iter, max_cells, flags, vp(status), vp(t),
                                         vp(xyz), vp(val), vp(grad), vp(evals), vp(cells))


def _fills(n):
    return (np.full(n, 7, np.uint8), np.full(n, 7.0), np.full((n, 3), 7.0), np.full(n, 7.0), np.full((n, 3), 7.0), np.full(n, 7, np.uint16),
            np.full(n, 7, np.uint16))


def test_null_optional_outputs(H):
    rng = np.random.default_rng(137)
    blk = dict(project_trees(rng))["max3"]
    rays = tuple(np.ascontiguousarray(a) for a in cast_rays(blk, rng, 64))
    n = len(rays[0])
    _, tol = cast_levels(H, blk, rng)
    full = H.cast_rays_block(blk, *rays, 0.0, tol, 32, 4096, True)
    for keep in range(1, 7):          # every optional output alone, the others NULL
        bufs = _fills(n)
        args = [bufs[i] if i == keep else None for i in range(1, 7)]
        assert _raw(H, blk, rays, n, 0.0, tol, 32, 4096, 1, bufs[0], *args) == H.OK
        assert np.array_equal(bufs[0], full[0])
        assert np.array_equal(_raw_bytes(bufs[keep]), _raw_bytes(full[keep])), keep
    bufs = _fills(n)
    assert _raw(H, blk, rays, n, 0.0, tol, 32, 4096, 1, bufs[0]) == H.OK and np.array_equal(bufs[0], full[0])


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(H):
    rng = np.random.default_rng(139)
    blk = dict(project_trees(rng))["max2-top"]
    rays = (rng.uniform(-0.4, 0.4, (4, 3)), rng.uniform(-1.0, 1.0, (4, 3)), np.full(4, 10.0))
    bufs = _fills(4)
    untouched = lambda: all((b == 7).all() for b in bufs)
    ok = dict(iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, flags=0)
    call = lambda n, r, a, b: _raw(H, blk, r, n, a["iso"], a["tol"], a["max_iter"], a["max_cells"], a["flags"], *b)
    assert call(0, rays, ok, bufs) == H.OK and untouched()
    assert call(0, (None, None, None), ok, (None,)) == H.OK
    bad = [dict(flags=2), dict(flags=0x80000001), dict(tol=-1e-300), dict(tol=float("nan")), dict(iso=float("inf")),
           dict(iso=float("-inf")), dict(iso=float("nan")), dict(max_iter=256), dict(max_iter=0xFFFFFFFF), dict(max_cells=0),
           dict(max_cells=65536), dict(max_cells=0xFFFFFFFF)]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        assert call(4, rays, a, bufs) == H.ERR_INVALID_ARGUMENT, kw
        assert H.lib().hpsdf_last_error() and untouched(), kw
    assert call(4, rays, dict(ok, flags=4), bufs) == H.ERR_INVALID_ARGUMENT and b"flag" in H.lib().hpsdf_last_error()
    assert call(4, rays, ok, (None,) + bufs[1:]) == H.ERR_INVALID_ARGUMENT and untouched()          # NULL out_status
    for missing in range(3):
        r = tuple(None if i == missing else rays[i] for i in range(3))
        assert call(4, r, ok, bufs) == H.ERR_INVALID_ARGUMENT and untouched(), missing
    assert call(4, rays, dict(ok, tol=0.0, max_iter=255, max_cells=65535, flags=1), bufs) == H.OK and not untouched()   # the limits pass
    bufs = _fills(4)
    for cut in (blk[:-1], blk[:100], blk[:8], b""):
        assert _raw(H, cut, rays, 4, 0.0, 1e-9, 32, 4096, 0, *bufs) == H.ERR_BAD_BLOCK and H.lib().hpsdf_last_error() and untouched()
    with pytest.raises(H.HpsdfError):
        H.cast_rays_block(blk[:-8], *rays)
    with pytest.raises(H.HpsdfError) as ei:
        H.cast_rays_block(blk, *rays, max_iter=300)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT
    with pytest.raises(H.HpsdfError):
        H.cast_rays_block(blk, *rays, max_cells=0)


def test_new_symbols_are_declared_bound_and_exported(H):
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_cast_rays_device", "hpsdf_cast_rays_host", "hpsdf_cast_rays_block"}
    assert new <= declared and new <= set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    assert int(re.search(r"#define HPSDF_CAST_UNIT (\d+)u", hdr).group(1)) == H.CAST_UNIT
    m = re.search(r"enum \{ HPSDF_CAST_HIT = (\d), HPSDF_CAST_MISS = (\d), HPSDF_CAST_UNCONVERGED = (\d), HPSDF_CAST_CELL_LIMIT = (\d), "
                  r"HPSDF_CAST_INVALID = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.CAST_HIT, H.CAST_MISS, H.CAST_UNCONVERGED, H.CAST_CELL_LIMIT, H.CAST_INVALID) == (0, 1, 2, 3, 4)
    assert (CR.HIT, CR.MISS, CR.UNCONVERGED, CR.CELL_LIMIT, CR.INVALID) == (0, 1, 2, 3, 4)
    assert H.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------------------ a built sphere
def _sphere_rays(rng, centre, radius, n):
    """n rays from outside the root [-0.5, 0.5]^3 that enter the sphere at a point inside the root with incidence |d . n| >= 0.5,
    |d| = 1 -> (origins, directions, analytic parameter t*)."""
    hits, dirs = [], []
    while len(hits) < n:
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        p = centre + radius * nrm
        if not (np.abs(p) <= 0.45).all():
            continue
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if v @ nrm > -0.55:           # incoming, with a margin over the 0.5 the bound's factor 2 stands for
            continue
        hits.append(p), dirs.append(v)
    hits, dirs = np.array(hits), np.array(dirs)
    org = hits - 2.0 * dirs
    assert (np.abs(org) > 0.5).any(1).all()
    # the analytic parameter from the origin itself: the smaller root of |o + t d - c|^2 = r^2
    oc = org - centre
    b = (oc * dirs).sum(1)
    t_star = -b - np.sqrt(b * b - ((oc * oc).sum(1) - radius * radius))
    assert (np.abs((dirs * (org + t_star[:, None] * dirs - centre)).sum(1)) / radius >= 0.5).all()
    return org, dirs, t_star


def test_sphere_first_crossing_reaches_the_fits_own_error(H, O):
    """The oracle's sphere tree at 1e-8 (centre (0.25, 0, 0), radius 0.5), 512 rays from outside the root with |d| = 1 and analytic
    incidence |d . n| >= 0.5, tol 1e-9, the default max_iter: every ray is a HIT; |t - t*| <= 4 E, t* the analytic ray-sphere parameter
    and E the largest |Query - F| at the 4096 points sampled along each ray on [t0, t) and at the hit itself (the 4: 2 for 1/|d . n|, 2
    for the fitted slope differing from 1); Query keeps one sign over those samples (the crossing found is the first); rays passing the
    sphere at 1.5 radii are MISS.  Measured when this was written: E = 1.77e-5, the largest |t - t*| 4.27e-6 (0.241 E), 28.6 evaluations
    and 6.3 leaves a ray on average, at most 60 evaluations."""
    tree = O.Tree.create(O.default_config(1e-8), O.sphere_field(), 1024)
    blk = tree.to_block()
    centre, radius, tol = np.array([0.25, 0.0, 0.0]), 0.5, 1e-9
    rng = np.random.default_rng(149)
    org, dirs, t_star = _sphere_rays(rng, centre, radius, 512)
    status, t, x, val, grad, evals, cells = H.cast_rays_block(blk, org, dirs, np.inf, 0.0, tol)
    assert (status == CR.HIT).all(), np.bincount(status, minlength=5)
    assert (np.abs(val) <= tol).all()
    # the entry parameter, as the header's clip computes it for a unit root
    with np.errstate(divide="ignore"):
        tin = np.where(dirs > 0, (-0.5 - org) / dirs, (0.5 - org) / dirs)
    t0 = np.maximum(0.0, tin.max(1))
    assert (t0 < t).all()
    s = t0[:, None] + (t - t0)[:, None] * (np.arange(4096) / 4096.0)[None, :]
    E, sign_changes = 0.0, 0
    for lo in range(0, 512, 64):
        sl = slice(lo, lo + 64)
        pts = org[sl, None, :] + s[sl, :, None] * dirs[sl, None, :]
        q = H.query_gradient_block(blk, pts.reshape(-1, 3))[0].reshape(64, 4096)
        inside = q != DBL_MAX            # (the first samples sit on the root's face and may round outside)
        assert inside[:, 8:].all()
        true = np.linalg.norm(pts - centre, axis=2) - radius
        E = max(E, float(np.abs(q - true)[inside].max()))
        neg = np.where(inside, q < 0, False)
        pos = np.where(inside, q >= 0, False)
        sign_changes += int((neg.any(1) & pos.any(1)).sum())
    E = max(E, float(np.abs(val - (np.linalg.norm(x - centre, axis=1) - radius)).max()))
    err = np.abs(t - t_star)
    print("E %.3g, max |t - t*| %.3g, ratio %.3g (bound 4), mean evals %.2f, mean cells %.2f, max evals %d"
          % (E, err.max(), err.max() / E, evals.mean(), cells.mean(), evals.max()))
    assert sign_changes == 0
    assert (err <= 4.0 * E).all(), (err.max(), E)
    assert_casts_equal((status, t, x, val, grad, evals, cells), CR.cast_reference(H, blk, org, dirs, np.inf, 0.0, tol), "sphere")
    # rays whose closest approach to the centre is 1.5 radii, inside the root: nothing to cross
    far_o, far_d = [], []
    while len(far_o) < 64:
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        p = centre + 1.5 * radius * nrm
        if not (np.abs(p) <= 0.45).all():
            continue
        v = np.cross(nrm, rng.normal(size=3))
        v /= np.linalg.norm(v)
        far_o.append(p - 2.0 * v), far_d.append(v)
    far = H.cast_rays_block(blk, np.array(far_o), np.array(far_d), np.inf, 0.0, tol)
    assert (far[0] == CR.MISS).all() and np.isnan(far[1]).all() and (far[6] >= 1).all()
