"""ExtractSurfaceDual without a device: hpsdf_extract_surface_dual_block (the statements of the kernels on the calling thread) against
the restatement of tests/dual_reference.py bit for bit, the invariants of every mesh, a built sphere, the sharp features of a built
box -- what the call exists for -- and the housekeeping of a new entry point."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import dual_reference as D
import hiprec as R
import surface_reference as S
from conftest import ROOT
from helpers import synthetic_block
from test_project_cpu import project_trees

SEED = 211
LATTICES = [(1, 1, 1), (2, 2, 2), (1, 17, 8), (16, 9, 1), (9, 8, 7), (65, 2, 2)]
TAUS = (0.0, 0.1, 0.5)
SPHERE_C, SPHERE_R = np.array([0.03, -0.02, 0.01]), 0.3
BOX_C, BOX_H = np.array([0.03, -0.02, 0.01]), np.array([0.21, 0.17, 0.25])
BOX_LO = np.array([-0.350625, -0.446875, -0.3275])
BOX_N = (12, 12, 12)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def inner_box(blk):
    """A lattice box strictly inside the block's root, off its mid-planes."""
    B = R.Block(blk)
    lo, hi = B.root_min.astype(np.float64), B.root_max.astype(np.float64)
    return lo + 0.031 * (hi - lo), hi - 0.047 * (hi - lo)


@pytest.fixture(scope="module")
def sphere_block(O):
    return O.Tree.create(O.default_config(1e-6), O.sphere_field(tuple(SPHERE_C), SPHERE_R), 1024).to_block()


@pytest.fixture(scope="module")
def box_block(O):
    field = O.AnalyticField([(O.PRIM_BOX, O.OP_UNION, list(BOX_C) + list(BOX_H))])
    return O.Tree.create(O.default_config(1e-7), field, 1024).to_block()


def box_distance(p):
    """Exact signed distance of the box at points p."""
    q = np.abs(np.asarray(p) - BOX_C) - BOX_H
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


def parity_cases(H, blk, lo, hi):
    """(n, iso, tau) of the parity tests: every lattice, iso 0 and the median lattice value, every tau."""
    for n in LATTICES:
        vals = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, values=True)[2]
        for iso in (0.0, float(np.median(vals))):
            for tau in TAUS:
                yield n, iso, tau, vals


def check_invariants(got, ref, n, what):
    verts, tris, info = got
    V, T = len(verts), len(tris)
    assert V == len(ref["cubes"]) and T == 2 * ref["interior"], what       # mixed cubes; 2 x interior crossing edges
    lo, hi, coords = ref["lo"], ref["hi"], ref["coords"]
    Q = ref["cubes"]
    idx = np.stack([Q % n[0], (Q // n[0]) % n[1], (Q // n[0]) // n[1]], axis=1)
    for a in range(3):
        assert (verts[:, a] >= coords[a][idx[:, a]]).all() and (verts[:, a] <= coords[a][idx[:, a] + 1]).all(), (what, a)
    assert ((info & 3) <= np.minimum(ref["k"], 3)).all() and (info & ~np.uint8(7) == 0).all(), what
    if T:
        assert int(tris.max()) < V, what
        # closedness, which always holds: a directed edge that its reverse does not balance joins two cubes across a face with an edge on
        # the lattice's boundary (boundary crossing edges give no quad) -- both cubes in the outer layer of an axis other than the face's
        e = Counter(map(tuple, S.directed_edges(tris).tolist()))
        for (u, w), c in e.items():
            if e.get((w, u), 0) == c:
                continue
            d = np.nonzero(idx[u] != idx[w])[0]
            assert len(d) == 1 and abs(int(idx[u][d[0]]) - int(idx[w][d[0]])) == 1, (what, u, w)
            assert any(idx[u][a] == 0 or idx[u][a] == n[a] - 1 for a in range(3) if a != d[0]), (what, u, w)


def run_parity(H, name, blk, lo, hi, left, lattices=None, stats=None):
    for n, iso, tau, vals in parity_cases(H, blk, lo, hi):
        if lattices is not None and n not in lattices:
            continue
        what = (name, left, n, iso, tau)
        ref = D.extract(H, blk, vals, lo, hi, n, iso, tau, left)
        verts, tris, info, v2 = H.extract_surface_dual_block(blk, lo, hi, n, iso, tau, values=True, info=True)
        assert np.array_equal(_bits(v2), _bits(vals)), what
        assert verts.shape == ref["verts"].shape and np.array_equal(_bits(verts), _bits(ref["verts"])), what
        assert tris.dtype == np.uint64 and np.array_equal(tris, ref["tris"]), what
        assert info.dtype == np.uint8 and np.array_equal(info, ref["info"]), what
        _, coords = S.lattice(lo, hi, n)
        ref.update(lo=lo, hi=hi, coords=coords)
        check_invariants((verts, tris, info), ref, n, what)
        if n == (1, 1, 1) and len(verts):
            assert len(verts) == 1 and len(tris) == 0, what
        if stats is not None:
            stats["residual"] = max([stats.get("residual", 0.0)] + ref["residuals"])
            stats["ranks"] = stats.get("ranks", set()) | set(int(r) for r in np.unique(info & 3))
            stats["clamped"] = stats.get("clamped", 0) + int(((info & 4) != 0).sum())
            stats["cubes"] = stats.get("cubes", 0) + len(verts)
            stats["open"] = stats.get("open", 0) + (1 if len(tris) and S.unmatched_edges(tris) else 0)


# ------------------------------------------------------------------------------------------------------------ parity and invariants
def test_block_entry_equals_the_restatement_bit_for_bit(H, sphere_block):
    """Synthetic blocks (degrees 0..12, discontinuous fields: degree-0 leaves give zero gradients and rank 0, ambiguous faces occur)
    and the oracle's sphere, every lattice, iso 0 and the median value, tau 0, 0.1 and 0.5; reduction order 1 on two lattices.
    Measured when this was written: 87 273 cubes, every rank 0..3 seen, 44 691 vertices clamped (the random fields of the synthetic
    blocks), 444 meshes open at the lattice's boundary."""
    rng = np.random.default_rng(SEED)
    before = H.reduction_order()
    stats = {}
    try:
        trees = [(name, blk) + inner_box(blk) for name, blk in project_trees(rng)]
        trees.append(("sphere", sphere_block, SPHERE_C - 0.35, SPHERE_C + 0.35))
        for name, blk, lo, hi in trees:
            H.set_reduction_order(0)
            run_parity(H, name, blk, lo, hi, 0, stats=stats)
            H.set_reduction_order(1)
            run_parity(H, name, blk, lo, hi, 1, lattices=[(2, 2, 2), (9, 8, 7)], stats=stats)
    finally:
        H.set_reduction_order(before)
    print("cubes %d, ranks %s, clamped %d, open meshes %d, largest Jacobi residual %.3g of the trace"
          % (stats["cubes"], sorted(stats["ranks"]), stats["clamped"], stats["open"], stats["residual"]))
    assert stats["ranks"] == {0, 1, 2, 3} and stats["clamped"] > 0 and stats["open"] > 0


def test_jacobi_sweeps_suffice(H, sphere_block, box_block):
    """HPSDF_DUAL_SWEEPS: after the last sweep the largest |off-diagonal| entry is at most 2^-40 of the trace on every cube of this
    file's tests -- the parity trees and lattices (through the restatement, whose bits are the block entry's), the sphere and the box.
    Measured when this was written: 2.6e-101 of the trace after 5 sweeps, 1.1e-24 after 4, 1.2e-6 after 3, 0.034 after 2 (2^-40 is
    9.1e-13: four sweeps would do, the fifth is the margin)."""
    rng = np.random.default_rng(SEED)
    worst = {s: 0.0 for s in (2, 3, 4, D.SWEEPS)}
    trees = [(blk,) + inner_box(blk) for _, blk in project_trees(rng)]
    cases = [(blk, lo, hi, n) for blk, lo, hi in trees for n in LATTICES]
    cases += [(sphere_block, SPHERE_C - 0.35, SPHERE_C + 0.35, n) for n in LATTICES + [(8, 8, 8), (16, 9, 5)]]
    cases.append((box_block, BOX_LO, BOX_LO + 0.75, BOX_N))
    for blk, lo, hi, n in cases:
        vals = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, values=True)[2]
        for iso in (0.0, float(np.median(vals))):
            for s in worst:
                worst[s] = max([worst[s]] + D.extract(H, blk, vals, lo, hi, n, iso, 0.1, H.reduction_order(), sweeps=s)["residuals"])
    print("largest residual over the trace by sweeps: %s" % {s: "%.3g" % w for s, w in worst.items()})
    assert D.SWEEPS == H.DUAL_SWEEPS == 5
    assert worst[D.SWEEPS] <= 2.0 ** -40


def test_closed_whenever_the_solid_lies_inside_the_lattice(H):
    """Random discontinuous fields with iso = the smallest value on the lattice's boundary, so that the solid {v < iso} lies inside the
    lattice, and just above the largest, so that its complement does: every directed edge has its reverse as often as it occurs itself (closedness, which always holds), and an edge that
    surface_reference.unmatched_edges reports is one that occurs more than once -- the non-manifold edge of an ambiguous face -- never
    an open one.  Where no edge repeats, unmatched_edges is empty."""
    rng = np.random.default_rng(SEED + 1)
    seen = repeated = 0
    for degrees in ([2, 1, 2, 2, 1, 2, 2, 1], [3, 2, 1, 0, 3, 3, 2, 1], [5, 4, 3, 2, 1, 0, 5, 4]):
        blk = synthetic_block(rng, degrees, 1)
        lo, hi = (-0.45,) * 3, (0.45,) * 3
        for n in [(9, 8, 7), (6, 6, 6), (16, 9, 5)]:
            vals = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, values=True)[2]
            shell = np.ones_like(vals, bool)
            shell[1:-1, 1:-1, 1:-1] = False
            # no boundary point has v < iso, or every one has: either way no boundary edge crosses
            for iso in (float(vals[shell].min()), float(np.nextafter(vals[shell].max(), np.inf))):
                verts, tris = H.extract_surface_dual_block(blk, lo, hi, n, iso, 0.1)
                if not len(tris):
                    continue
                seen += 1
                e = Counter(map(tuple, S.directed_edges(tris).tolist()))
                assert all(e.get((b, a), 0) == c for (a, b), c in e.items()), (degrees, n, iso)
                bad = S.unmatched_edges(tris)
                assert all(e[k] > 1 for k in bad), (degrees, n, iso)
                repeated += 1 if bad else 0
    print("%d closed meshes, %d of them with a non-manifold edge" % (seen, repeated))
    assert seen >= 2


# ------------------------------------------------------------------------------------------------------------ the sphere
@pytest.mark.parametrize("n", [(9, 8, 7), (8, 8, 8), (16, 9, 5)])
def test_sphere_is_closed_and_close(H, O, sphere_block, n):
    """The oracle's sphere at 1e-6 over [c - 0.35, c + 0.35]: no unmatched edges, one component, Euler characteristic 2, positive
    volume, and every vertex within |h|_2 + E of the true sphere -- it lies in a cube the fitted surface crosses -- E being the largest
    |Query - F| over the lattice points.  Measured when this was written: the largest distance is 0.091, 0.092 and 0.083 of the largest
    cube edge for the three lattices (E = 8.5e-4, 1.5e-2 and 1.1e-3: the fit is coarsest near the sphere's centre); every vertex has
    rank 1."""
    lo, hi = SPHERE_C - 0.35, SPHERE_C + 0.35
    verts, tris, info, vals = H.extract_surface_dual_block(sphere_block, lo, hi, n, 0.0, 0.1, values=True, info=True)
    assert S.unmatched_edges(tris) == [] and S.components(tris) == 1 and S.euler_characteristic(verts, tris) == 2
    assert S.signed_volume(verts, tris) > 0
    h = 0.7 / np.array(n, np.float64)
    P = S.lattice_points(lo, hi, n)
    E = float(np.abs(vals.ravel() - (np.linalg.norm(P - SPHERE_C, axis=1) - SPHERE_R)).max())
    d = np.abs(np.linalg.norm(verts - SPHERE_C, axis=1) - SPHERE_R)
    print("n %s: V %d T %d, E %.3g, largest distance %.3g = %.3f h_max, ranks %s" % (n, len(verts), len(tris), E, d.max(), d.max() / h.max(),
                                                                                   np.bincount(info & 3, minlength=4).tolist()))
    assert d.max() <= np.linalg.norm(h) + E


# ------------------------------------------------------------------------------------------------------------ sharp features
def box_checks(H, verts, tris, info, mc_verts):
    """Assertions (a)-(e) of the sharp-feature test on a dual mesh of the box (shared with the GPU test)."""
    h = 0.75 / 12
    corners = np.array([[BOX_C[a] + (1 if (c >> a) & 1 else -1) * BOX_H[a] for a in range(3)] for c in range(8)])
    _, coords = S.lattice(BOX_LO, BOX_LO + 0.75, BOX_N)
    dual_d, mc_d, edge_d = [], [], []
    for c in corners:
        d = np.linalg.norm(verts - c, axis=1)
        v = int(d.argmin())
        dual_d.append(d[v])
        assert d[v] <= 0.25 * h and (info[v] & 3) == 3, (c, d[v] / h, int(info[v]))                         # (a)
        # the corner's distance to the nearest lattice edge: along axis a an edge sits at lattice coordinates of the other two axes
        off = [np.abs(coords[a] - c[a]).min() for a in range(3)]
        edge = min(np.hypot(off[(a + 1) % 3], off[(a + 2) % 3]) for a in range(3))
        m = np.linalg.norm(mc_verts - c, axis=1).min()
        mc_d.append(m)
        edge_d.append(edge)
        # (b): a marching-cubes vertex lies on a lattice edge, so none is nearer than the nearest edge -- and that is farther than (a)'s bound
        assert m >= edge > 0.25 * h, (c, m / h, edge / h)
    surf = np.abs(box_distance(verts))
    assert surf.max() <= 0.25 * h, surf.max() / h                                                           # (c)
    vol, exact = S.signed_volume(verts, tris), 8.0 * BOX_H.prod()
    assert abs(vol - exact) <= 0.01 * exact, vol / exact                                                    # (d)
    assert S.unmatched_edges(tris) == [] and S.euler_characteristic(verts, tris) == 2                       # (e)
    return dict(dual=np.array(dual_d) / h, mc=np.array(mc_d) / h, edge=np.array(edge_d) / h, surface=surf.max() / h, volume=vol / exact - 1.0)


def test_box_keeps_its_corners_where_marching_cubes_cuts_them(H, box_block):
    """The oracle's box (centre (0.03, -0.02, 0.01), half extents (0.21, 0.17, 0.25)) at 1e-7 on a 12^3 lattice with h = 1/16, tau 0.1:
    (a) each of the 8 exact corners has a dual vertex of rank 3 within 0.25 h; (b) the nearest marching-cubes vertex is no closer than
    the corner's distance to the nearest lattice edge, computed from the geometry, which exceeds (a)'s 0.25 h at every corner; (c) every dual vertex lies within 0.25 h of the exact
    box; (d) the volume is within 1 %; (e) closed with Euler characteristic 2.
    Measured through the block entry when this was written: the nearest dual vertex 0.0006 .. 0.0864 h from its corner, the nearest
    marching-cubes vertex 0.516 .. 0.755 h (the nearest lattice edge 0.292 .. 0.602 h: not >= 0.5 h at every corner, as the request for
    this test supposed, but above 0.25 h at each), the largest |exact distance| of a dual vertex 0.1191 h, the volume 0.499 % too
    large, V 264, T 524, ranks 188 x 1, 68 x 2, 8 x 3 -- a factor of two or more inside every bound."""
    lo, hi = BOX_LO, BOX_LO + 0.75
    verts, tris, info, vals = H.extract_surface_dual_block(box_block, lo, hi, BOX_N, 0.0, 0.1, values=True, info=True)
    mc_verts, _ = S.extract(vals, lo, hi, BOX_N, 0.0, H.surface_case_table())
    m = box_checks(H, verts, tris, info, mc_verts)
    print("corner -> nearest dual vertex %.4f..%.4f h, -> nearest marching-cubes vertex %.3f..%.3f h (nearest lattice edge %.3f..%.3f h), "
          "largest |exact distance| of a dual vertex %.4f h, volume off by %.3f %%, V %d T %d, ranks %s"
          % (m["dual"].min(), m["dual"].max(), m["mc"].min(), m["mc"].max(), m["edge"].min(), m["edge"].max(), m["surface"],
             100 * m["volume"], len(verts), len(tris), np.bincount(info & 3, minlength=4).tolist()))


# ------------------------------------------------------------------------------------------------------------ housekeeping
def _raw(H, block, lo, hi, n, iso, tau, flags, want_info=True, values=None):
    buf = bytes(block)
    v, t, b = C.POINTER(C.c_double)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
    nv, nt = C.c_uint64(77), C.c_uint64(77)
    d3 = lambda x: (C.c_double * 3)(*x)
    rc = H.lib().hpsdf_extract_surface_dual_block(buf, len(buf), d3(lo), d3(hi), (C.c_uint32 * 3)(*n), iso, tau, flags, C.byref(v), C.byref(nv),
                                                  C.byref(t), C.byref(nt), C.byref(b) if want_info else None,
                                                  None if values is None else values.ctypes.data_as(C.c_void_p))
    out = (rc, nv.value, nt.value, bool(v), bool(t), bool(b))
    for p in (v, t, b):
        H.lib()._libc.free(C.cast(p, C.c_void_p))
    return out


def test_argument_checks(H):
    rng = np.random.default_rng(SEED + 2)
    blk = synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)
    lo, hi, n = (-0.4,) * 3, (0.4,) * 3, (4, 4, 4)
    ok = _raw(H, blk, lo, hi, n, 0.0, 0.1, 0)
    assert ok[0] == H.OK and ok[1] > 0 and ok[3] and ok[5]
    nothing = (0, 0, False, False, False)
    bad = [dict(tau=-1e-300), dict(tau=1.0), dict(tau=2.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=float("-inf")),
           dict(flags=1), dict(flags=0x80000000), dict(iso=float("nan")), dict(iso=float("inf")), dict(n=(0, 4, 4)), dict(hi=(0.4, 0.4, 0.6)),
           dict(lo=(0.4, -0.4, -0.4)), dict(hi=(0.4, float("nan"), 0.4))]
    for kw in bad:
        a = dict(lo=lo, hi=hi, n=n, iso=0.0, tau=0.1, flags=0)
        a.update(kw)
        got = _raw(H, blk, a["lo"], a["hi"], a["n"], a["iso"], a["tau"], a["flags"])
        assert got[0] == H.ERR_INVALID_ARGUMENT and got[1:] == nothing and H.lib().hpsdf_last_error(), kw
    assert _raw(H, blk, lo, hi, n, 0.0, 0.0, 0)[0] == H.OK and _raw(H, blk, lo, hi, n, 0.0, np.nextafter(1.0, 0.0), 0)[0] == H.OK  # the limits pass
    for cut in (blk[:-1], blk[:100], blk[:8], b""):
        got = _raw(H, cut, lo, hi, n, 0.0, 0.1, 0)
        assert got[0] == H.ERR_BAD_BLOCK and got[1:] == nothing and H.lib().hpsdf_last_error()
    with pytest.raises(H.HpsdfError) as ei:
        H.extract_surface_dual_block(blk, lo, hi, n, tau=1.5)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT
    with pytest.raises(H.HpsdfError):
        H.extract_surface_dual_block(blk[:-8], lo, hi, n)


def test_null_optional_outputs_and_the_empty_result(H):
    rng = np.random.default_rng(SEED + 3)
    blk = synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)
    lo, hi, n = (-0.4,) * 3, (0.4,) * 3, (5, 4, 3)
    full = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, values=True, info=True)
    bare = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1)
    assert len(bare) == 2 and np.array_equal(_bits(bare[0]), _bits(full[0])) and np.array_equal(bare[1], full[1])
    only_info = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, info=True)
    only_vals = H.extract_surface_dual_block(blk, lo, hi, n, 0.0, 0.1, values=True)
    assert np.array_equal(only_info[2], full[2]) and np.array_equal(_bits(only_vals[2]), _bits(full[3]))
    got = _raw(H, blk, lo, hi, n, 0.0, 0.1, 0, want_info=False)
    assert got[0] == H.OK and got[1] == len(full[0]) and got[2] == len(full[1]) and not got[5]
    # an empty result: iso below every value -- HPSDF_OK, counts 0, NULL pointers, the values still written
    vals = np.full(full[3].shape, 7.0)
    got = _raw(H, blk, lo, hi, n, float(full[3].min()) - 1.0, 0.1, 0, values=vals)
    assert got == (H.OK, 0, 0, False, False, False) and np.array_equal(_bits(vals), _bits(full[3]))
    e = H.extract_surface_dual_block(blk, lo, hi, n, float(full[3].min()) - 1.0, 0.1, info=True)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,)
    # vertices without a triangle: a single cube
    one = H.extract_surface_dual_block(blk, (-0.4,) * 3, (0.37,) * 3, (1, 1, 1), float(np.median(full[3])), 0.1, info=True)
    if len(one[0]):
        assert one[0].shape == (1, 3) and one[1].shape == (0, 3) and one[2].shape == (1,)
    got = _raw(H, blk, (-0.4,) * 3, (0.37,) * 3, (1, 1, 1), float(np.median(full[3])), 0.1, 0)
    assert got[0] == H.OK and got[2] == 0 and not got[4] and got[3] == (got[1] == 1)


def test_single_cube_gives_one_vertex_and_no_triangle(H, sphere_block):
    """(1,1,1) across the sphere's surface: V = 1, T = 0, and the vertex comes back."""
    lo = SPHERE_C + np.array([SPHERE_R - 0.02, -0.03, -0.03])
    verts, tris, info = H.extract_surface_dual_block(sphere_block, lo, lo + 0.05, (1, 1, 1), 0.0, 0.1, info=True)
    assert verts.shape == (1, 3) and tris.shape == (0, 3) and info.shape == (1,)
    assert (verts[0] >= lo).all() and (verts[0] <= lo + 0.05).all()


def test_new_symbols_are_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_extract_surface_dual", "hpsdf_extract_surface_dual_block", "hpsdf_surface_dual_last_timings"}
    assert new <= declared and new <= set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    assert int(re.search(r"#define HPSDF_DUAL_SWEEPS (\d+)", hdr).group(1)) == H.DUAL_SWEEPS
    assert int(re.search(r"#define HPSDF_DUAL_CLAMPED (\d+)u", hdr).group(1)) == H.DUAL_CLAMPED
    assert H.ABI_VERSION == 4 and H.lib().hpsdf_abi_version() == 4
    assert hasattr(H.DeviceTree, "extract_surface_dual") and hasattr(H, "extract_surface_dual_block") and hasattr(H, "surface_dual_last_timings")
    cxx = open(os.path.join(ROOT, "include", "hpsdf_octree.hpp")).read()
    assert "ExtractSurfaceDual" in cxx


def test_dual_does_not_combine_with_sparse_or_project(H, sphere_block):
    oct = H.Octree()
    oct._tree = object()  # (a tree needs a device; the refusal comes before the tree is touched)
    try:
        for kw in (dict(sparse=True), dict(project=True), dict(sparse=True, normals=True), dict(project=True, curvature=True)):
            with pytest.raises(ValueError):
                oct.ExtractSurface((-0.4,) * 3, (0.4,) * 3, 8, dual=True, **kw)
    finally:
        oct._tree = None
