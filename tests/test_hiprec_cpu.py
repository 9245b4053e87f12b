"""The extended-precision reference (tests/hiprec.py) on the CPU: the reference's tables against mathematics, the reference
against a 40-digit evaluation, the oracle's fits and queries within the derived bounds, and mutants of the operation that
the bounds reject."""
from math import comb

import mpmath
import numpy as np
import pytest

import hiprec as R
from helpers import deep_chain_block, synthetic_block

ROOTS = {"unit": ((-0.5,) * 3, (0.5,) * 3), "cube": ((-0.25,) * 3, (5.0,) * 3), "aniso": ((-2.0, -0.125, 0.0), (6.0, 0.125, 1.0))}


# ------------------------------------------------------------------------------------------------------------ tables
def _mp_legendre(n, x):
    """P_n(x) and P_n'(x) by the textbook recurrence, in mpmath (the same polynomial as mpmath.legendre, much faster)."""
    p0, p1 = mpmath.mpf(1), x
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    return p1, n * (x * p1 - p0) / (x * x - 1)


def test_gauss_rules_are_the_legendre_rules():
    """Every rule the table holds (orders 1..64): each node is a root of P_n correctly rounded, each weight 2/((1-x^2) P_n'(x)^2)
    correctly rounded -- Newton on P_n from the float64 node at 40 digits.  The reference deviates nowhere."""
    with mpmath.workdps(40):
        assert mpmath.almosteq(_mp_legendre(7, mpmath.mpf("0.3"))[0], mpmath.legendre(7, mpmath.mpf("0.3")), 1e-35)
        bad = []
        for n in range(1, 65):
            xs, ws = R.rule(n)
            for q in range(n):
                x = mpmath.mpf(float(xs[q]))
                for _ in range(4):
                    p, d = _mp_legendre(n, x)
                    x -= p / d
                p, d = _mp_legendre(n, x)
                w = 2 / ((1 - x * x) * d * d)
                if float(x) != xs[q] or float(w) != ws[q]:
                    bad.append((n, q))
    assert bad == []
    assert np.array_equal(R.SUMTON, np.arange(50) * (np.arange(50) + 1) // 2)


# NormalisedLengths = SqrtConst((2i + 1) 2^j), 100 Newton steps from x (Utility.h): these entries are 1 ulp off the correctly
# rounded square root.  A property of the reference that parity keeps, not a defect.
NL_ULP_OFF = ([(0, j) for j in (1, 3, 5, 7, 9)] + [(2, j) for j in (1, 3, 5, 7, 9)] + [(4, j) for j in (1, 3, 5, 7, 9)]
              + [(6, j) for j in (0, 2, 4, 6, 8, 10)] + [(9, j) for j in range(11)])


def test_small_tables_against_mathematics():
    off = []
    with mpmath.workdps(40):
        for i in range(13):
            for j in range(11):
                true = mpmath.sqrt((2 * i + 1) * 2 ** j)
                if R.NL[i, j] != float(true):
                    off.append((i, j))
                    assert abs(mpmath.mpf(float(R.NL[i, j])) - true) <= np.spacing(R.NL[i, j]), (i, j)
    assert off == NL_ULP_OFF
    assert R.REC[0].tolist() == [0.0, 0.0]
    for j in range(1, 13):
        assert R.REC[j].tolist() == [(2 * j - 1) / j, (j - 1) / j]    # correctly rounded quotients
    # (1.0/6) (p+1)(p+2)(p+3) truncated: the degree-6 basis has 83 functions, not C(9, 3) = 84
    assert [(p, int(R.COUNT[p])) for p in range(13) if R.COUNT[p] != comb(p + 3, 3)] == [(6, 83)]
    # BasisIndexValues: by total degree, then i, then j; the degree-6 block simply stops one short
    want = [(i, j, p - i - j) for p in range(13) for i in range(p + 1) for j in range(p - i + 1)]
    assert [tuple(r) for r in R.BIDX.tolist()] == want[:455] and len(want) == 455
    for p in range(13):
        assert R.BIDX[:R.COUNT[p]].sum(1).max() <= p
    assert R.BIDX[:83].sum(1).tolist() == sorted(R.BIDX[:83].sum(1).tolist())
    assert int((R.BIDX[:83].sum(1) == 6).sum()) == 27   # 28 functions of degree 6 exist


def test_recurrence_error_model():
    """The bound's model for Octree::LpX in float64: |L_j - L*_j| <= j^2 u, at every node of every rule a fit uses and at the
    gradient's offset points x +- 1e-4 on [-1, 1]."""
    xs = [R.rule(4 * p + 1)[0] for p in range(1, 12)] + [np.linspace(-1 - R.H_GRAD, 1 + R.H_GRAD, 4001)]
    x = np.concatenate(xs)
    got, want = R.legendre_f64(x, 12), R.legendre_ld(x, 12)
    err = np.abs(got.astype(R.LD) - want).astype(np.float64)
    j2 = np.maximum(np.arange(13), 1)[:, None] ** 2
    assert (err <= j2 * R.U).all(), (err / (j2 * R.U)).max()


# ------------------------------------------------------------------------------------------------------------ fits
def _mp_fit(spec, root, bmin, bmax, degree, depth, rows):
    """The fit of `rows` at 40 digits: the same float64 sample positions, everything after them in mpmath."""
    mp = mpmath.mpf
    nq = 4 * degree + 1
    x, w = R.rule(nq)
    scale = (bmax - bmin).astype(np.float64) * 0.5
    centre = ((bmin + bmax) / np.float32(2.0)).astype(np.float64)
    rmin, rmax = np.asarray(root[0], np.float32), np.asarray(root[1], np.float32)
    rb, rc = (rmax - rmin).astype(np.float64), ((rmin + rmax) / np.float32(2.0)).astype(np.float64)
    W = [(x * scale[a] + centre[a]) * rb[a] + rc[a] for a in range(3)]

    def prim(kind, p, X):
        d = [mp(X[a]) - mp(p[a]) for a in range(3)]
        if kind == R.PRIM_SPHERE:
            return mpmath.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) - mp(p[3])
        if kind == R.PRIM_BOX:
            q = [abs(d[a]) - mp(p[3 + a]) for a in range(3)]
            return mpmath.sqrt(sum(max(v, 0) ** 2 for v in q)) + min(max(q), 0)
        if kind == R.PRIM_TORUS_Y:
            l = mpmath.sqrt(d[0] ** 2 + d[2] ** 2) - mp(p[3])
            return mpmath.sqrt(l * l + d[1] ** 2) - mp(p[4])
        return mp(p[0]) * mp(X[0]) + mp(p[1]) * mp(X[1]) + mp(p[2]) * mp(X[2]) + mp(p[3])

    F = np.empty((nq, nq, nq), object)
    for i in range(nq):
        for j in range(nq):
            for k in range(nq):
                X = (W[0][i], W[1][j], W[2][k])
                acc = None
                for kind, op, p in spec:
                    v = prim(kind, p, X)
                    acc = v if acc is None else min(acc, v) if op == R.OP_UNION else max(acc, v) if op == R.OP_INTERSECT else max(acc, -v)
                F[i, j, k] = acc
    L = np.empty((degree + 1, nq), object)
    for q in range(nq):
        m2, m1, xx = mp(0), mp(1), mp(x[q])
        L[0, q] = mp(1) * mp(w[q])
        for a in range(1, degree + 1):
            li = mp(R.REC[a][0]) * xx * m1 - mp(R.REC[a][1]) * m2
            m2, m1 = m1, li
            L[a, q] = li * mp(w[q])
    G1 = np.tensordot(L, F, axes=([1], [0]))                    # [a, j, k]
    S = mp(scale[0]) * mp(scale[1]) * mp(scale[2])
    out = []
    for r in rows:
        a, b, c = R.BIDX[r]
        g2 = np.tensordot(L[b], G1[a], axes=([0], [0]))          # [k]
        v = np.dot(L[c], g2)
        out.append(S * mp(R.NL[a, depth]) * mp(R.NL[b, depth]) * mp(R.NL[c, depth]) * v)
    return out


def test_reference_agrees_with_40_digits():
    """Degree 11 on a kinked cell (a box's corner carved by a sphere and a torus), every row: the long-double reference is
    within bound/64 of a 40-digit evaluation of the same operation."""
    root = ROOTS["cube"]
    depth, degree = 3, 11
    spec = R.corner_fields(*root, depth)["carve"]
    bmin, bmax = R.lattice_cells(depth, 1)
    ref = R.fit_reference(spec, *root, bmin, bmax, degree, depth)
    rows = list(range(int(R.COUNT[degree])))
    with mpmath.workdps(40):
        want = _mp_fit(spec, root, bmin[0], bmax[0], degree, depth, rows)
        err = np.array([float(abs(mpmath.mpf(float(ref["c"][0, r])) + mpmath.mpf(float(ref["c"][0, r] - R.LD(float(ref["c"][0, r]))))
                                  - want[r])) for r in rows])
    assert (err <= ref["bound"][0] / 64).all(), (err / ref["bound"][0]).max()


def _cpu_cases():
    """Degrees 2..11, all three roots, every depth 0..10 met by every root."""
    out = []
    for ri, root in enumerate(ROOTS):
        for p in range(2, 12):
            for depth in sorted({(p + 4 * ri) % 11, (p + 5 + ri) % 11}):
                out.append((root, p, depth))
    return out


def test_case_grid_covers_every_depth():
    cases = _cpu_cases()
    for root in ROOTS:
        assert {d for r, _, d in cases if r == root} == set(range(11))
    assert {p for _, p, _ in cases} == set(range(2, 12))


@pytest.mark.parametrize("left", [False, True])
def test_oracle_fits_within_the_bounds(O, left):
    """ora_fit_polynomial -- the exact mode's bits -- lies within the bounds, coefficients and error, on cells holding a sphere's
    surface, a box's corner, a union's crease, a CSG carve and a plane (the plane's rows above degree 1 vanish: the bound must hold
    at zero too), in both reduction orders."""
    worst = 0.0
    O.set_reduction_order(1 if left else 0)
    try:
        for k, (root, p, depth) in enumerate(_cpu_cases()):
            if left and k % 3:
                continue
            rmin, rmax = ROOTS[root]
            cfg = O.default_config(1e-5, rmin, rmax)
            fields = R.corner_fields(rmin, rmax, depth)
            names = list(fields) if p <= 7 else [list(fields)[k % 5], "plane"]
            ncell = 2 if depth else 1
            bmin, bmax = R.lattice_cells(depth, ncell)
            for name in names:
                ref = R.fit_reference(fields[name], rmin, rmax, bmin, bmax, p, depth, left)
                got = [O.fit_polynomial(O.AnalyticField(fields[name]), cfg, bmin[i], bmax[i], p, depth) for i in range(ncell)]
                rc, re = R.fit_ratio(ref, np.array([g[0] for g in got]), np.array([g[1] for g in got]))
                assert rc <= 1 and re <= 1, (root, p, depth, name, rc, re)
                worst = max(worst, rc, re)
    finally:
        O.set_reduction_order(0)
    assert worst > 0


def _mutants(spec, root, bmin, bmax, p, depth, kinked):
    nq = 4 * p + 1
    out = {"samples_f32": R.fit_reference(spec, *root, bmin, bmax, p, depth, samples_f32=True),
           "zero_weight": R.fit_reference(spec, *root, bmin, bmax, p, depth, zero_sample=(1, nq // 2 - 1, nq - 3))}
    if kinked:
        out["gauss_4p-1"] = R.fit_reference(spec, *root, bmin, bmax, p, depth, order=4 * p - 1)
    for dd in (-1, 1):
        if 0 <= depth + dd <= 10:
            out["nl_depth%+d" % dd] = R.fit_reference(spec, *root, bmin, bmax, p, depth, nl_depth=depth + dd)
    return out


@pytest.mark.parametrize("p", [2, 3, 5, 8, 11])
def test_fit_bounds_reject_the_mutants(p):
    """Each mutant of the operation breaks the bound in at least one coefficient of every case it applies to: samples rounded to
    float32; one sample's weight zeroed; the Gauss order 4p - 1 instead of 4p + 1 (on cells with a kink); NormalisedLengths at
    depth - 1 and depth + 1.  A bound loose enough to admit one of these would fail here."""
    seen = set()
    for ri, (root, (rmin, rmax)) in enumerate(ROOTS.items()):
        depth = (p + 3 * ri) % 11
        fields = R.corner_fields(rmin, rmax, depth)
        bmin, bmax = R.lattice_cells(depth, 1)
        for name in ("sphere", "box", "crease", "plane"):
            true = R.fit_reference(fields[name], rmin, rmax, bmin, bmax, p, depth)
            for mname, mut in _mutants(fields[name], (rmin, rmax), bmin, bmax, p, depth, name in ("box", "crease")).items():
                excess = (np.abs(mut["c"] - true["c"]).astype(np.float64) / true["bound"]).max()
                assert excess > 1, (root, depth, name, mname, excess)
                seen.add(mname)
    assert {"samples_f32", "zero_weight", "gauss_4p-1", "nl_depth-1", "nl_depth+1"} <= seen


# ------------------------------------------------------------------------------------------------------------ query
def _with_root(blk, rmin, rmax):
    """A block with another root in its config (the last 80 bytes: root_min @56, root_max @68)."""
    b = bytearray(blk)
    b[-24:] = np.array(list(rmin) + list(rmax), np.float32).tobytes()
    return bytes(b)


def query_blocks(rng):
    """Synthetic blocks: every degree 0..12 and every depth 0..10 (deep_chain_block), on the unit root and on [-0.25, 5]^3."""
    out = []
    for rmin, rmax in (ROOTS["unit"], ROOTS["cube"]):
        out.append(("syn0-7", synthetic_block(rng, list(range(8)), 1, rmin, rmax)))
        out.append(("syn8-12", synthetic_block(rng, [8, 9, 10, 11, 12, 12, 11, 10], 2, rmin, rmax)))
        out.append(("chain", _with_root(deep_chain_block(rng, 10, degrees=tuple(range(13))), rmin, rmax)))
    return out


def test_query_blocks_cover_every_degree_and_depth():
    blocks = [R.Block(b) for _, b in query_blocks(np.random.default_rng(5))]
    assert set().union(*({int(v) for v in b.degree[b.leaves()]} for b in blocks)) == set(range(13))
    assert set().union(*({int(v) for v in b.depth[b.leaves()]} for b in blocks)) == set(range(1, 11))


def test_oracle_query_within_the_bounds(O):
    """Tree.query and query_with_gradient of the oracle at points strictly inside leaves, against the Query bounds: the value,
    and the normalised central-difference gradient with its 1/(2h) amplification."""
    rng = np.random.default_rng(11)
    for name, blk in query_blocks(rng):
        pts = R.points_in_leaves(blk, rng, 400)
        ref = R.fapprox_reference(blk, pts, gradient=True)
        t = O.Tree.from_block(blk)
        v = t.query(pts)
        vg, g = t.query_with_gradient(pts)
        assert np.array_equal(v, vg)
        rv = (np.abs(v.astype(R.LD) - ref["f"]).astype(np.float64) / ref["f_bound"]).max()
        rg = (np.abs(g.astype(R.LD) - ref["g"]).astype(np.float64) / ref["g_bound"]).max()
        assert rv <= 1 and rg <= 1, (name, rv, rg)


def test_query_bound_rejects_a_perturbed_recurrence():
    """One recurrence coefficient 64 ulp off (rec[1][0] = 1 + 64 * 2^-52): at leaves of degree 1..3 the mutant's Query leaves
    the bound somewhere in every block.  (Higher degrees add terms to the bound faster than this perturbation grows.)"""
    rng = np.random.default_rng(13)
    rec = R.REC.copy()
    rec[1][0] = 1.0 + 64 * 2.0 ** -52
    for rmin, rmax in (ROOTS["unit"], ROOTS["cube"]):
        for degs in ([1] * 8, [2] * 8, [3] * 8):
            blk = synthetic_block(rng, degs, 1, rmin, rmax)
            pts = R.points_in_leaves(blk, rng, 200)
            true, mut = R.fapprox_reference(blk, pts), R.fapprox_reference(blk, pts, rec=rec)
            excess = (np.abs(mut["f"] - true["f"]).astype(np.float64) / true["f_bound"]).max()
            assert excess > 1, (degs[0], excess)
