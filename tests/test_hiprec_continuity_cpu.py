"""The extended-precision continuity reference (tests/hiprec_continuity.py) on the CPU: the reference against mathematics,
the oracle's and the product's host matrix within its entry bounds, mutants of the operation that the bounds reject, and both
conjugate-gradient loops (oracle, product host) against the true residual and a long-double solve."""
import hashlib
import itertools

import numpy as np
import pytest

import hiprec as R
import hiprec_continuity as RC
from helpers import deep_chain_block, oracle_field, synthetic_block

LD = R.LD
STRENGTH = 8.0
EIGHT = [4, 1, 0, 6, 2, 2, 9, 3]
MIXED = [12, 0, 7, 3, 11, 2, 5, 9]
BUILT = ("union3", 3e-6, 1024)            # the smallest of the usual targets at which union3 refines: depths 4 and 5, degrees 2 and 3
SYNTHETIC = ("eight", "mixed", "chain4", "chain10")


def multiple_of_256():
    """The first eight-leaf degree set (non-decreasing, lexicographic) whose coefficient count is a multiple of 256."""
    for degs in itertools.combinations_with_replacement(range(13), 8):
        if int(R.COUNT[list(degs)].sum()) % 256 == 0:
            return list(degs)
    return None


def synthetic_case(name):
    rng = np.random.default_rng(11)
    if name == "eight":
        blk = synthetic_block(rng, EIGHT, depth=1)
    elif name == "mixed":
        blk = synthetic_block(rng, MIXED, depth=2)
    elif name == "chain4":
        blk = deep_chain_block(rng, max_depth=4)
    elif name == "chain10":
        blk = deep_chain_block(rng, max_depth=10)
    elif name == "x256":
        blk = synthetic_block(rng, multiple_of_256(), depth=1)
    else:
        raise KeyError(name)
    return RC.with_strength(blk, STRENGTH)


_REFS = {}


def _key(name, blk):
    return name, hashlib.sha1(bytes(blk)).hexdigest()


def ref_of(name, blk):
    """One reference matrix per block and test session (keyed by the block's bytes: the GPU module shares the cache, and its
    built tree comes from another Create)."""
    k = _key(name, blk)
    if k not in _REFS:
        _REFS[k] = RC.reference(blk)
    return _REFS[k]


@pytest.fixture(scope="module")
def blocks(O):
    out = {name: synthetic_case(name) for name in SYNTHETIC}
    cfg = O.default_config(BUILT[1])
    cfg.continuity_strength = STRENGTH
    out["built"] = O.Tree.create(cfg, oracle_field(O, BUILT[0]), BUILT[2]).to_block()
    return out


# ------------------------------------------------------------------------------------------------------------ models
def test_recurrence_model_at_face_arguments():
    """Section 2 (i): Octree::LpX in float64 with the table's rounded coefficients against the Legendre polynomials, |dL_j| <= j^2 u,
    at +-1, at every node of the rules a face uses and at those nodes moved onto every sub-face of depth differences 1..9."""
    xs = [np.array([-1.0, 1.0])]
    for n in range(1, 14):
        r = R.rule(n)[0]
        xs.append(r)
        for k in range(1, 10):
            inv = 2.0 ** -k
            for t in {-(1 - inv), 1 - inv, inv if k > 1 else 0.5, -3 * inv if k > 1 else -0.5}:
                xs.append(r * inv + t)
    x = np.concatenate(xs)
    assert np.abs(x).max() <= 1
    err = np.abs(R.legendre_f64(x, 12).astype(LD) - RC.legendre(x.astype(LD), 12)).astype(np.float64)
    j2 = np.maximum(np.arange(13), 1)[:, None] ** 2
    assert (err <= j2 * R.U).all(), (err / (j2 * R.U)).max()
    d = np.abs(np.gradient(RC.legendre(np.linspace(-1, 1, 4001).astype(LD), 12).astype(np.float64), 2 / 4000, axis=1))
    assert (d.max(1) <= np.arange(13) * (np.arange(13) + 1) / 2 * (1 + 1e-3)).all()          # |L_j'| <= j (j + 1) / 2


def test_long_double_rules_are_exact_and_round_to_the_table():
    for n in range(1, 14):
        x, w = RC.rule_ld(n)
        for exact, table in ((x, R.rule(n)[0]), (w, R.rule(n)[1])):                       # the table: these, correctly rounded
            assert (np.abs(exact - table.astype(LD)).astype(np.float64) <= R.U * np.abs(table) * (1 + 2.0 ** -9)).all(), n
        for k in range(2 * n):
            want = LD(0) if k % 2 else LD(2) / (k + 1)
            assert abs((w * x ** k).sum() - want) <= 2.0 ** -60, (n, k)
    for i, j in R.BIDX[:40, :2]:
        assert abs(RC.NL_LD[i, j] ** 2 - (2 * int(i) + 1) * 2 ** int(j)) <= 2.0 ** -60 * (2 * int(i) + 1) * 2 ** int(j)
    assert (np.abs(RC.NL_LD.astype(np.float64) - R.NL) <= np.spacing(R.NL)).all()           # K_NL: one ulp


# ------------------------------------------------------------------------------------------------------------ mathematics
def _project(blk, g):
    """The exact L2 projection of a polynomial g(x, y, z) (root-normalised coordinates, long double) into every leaf."""
    b = R.Block(blk)
    x, w = RC.rule_ld(13)
    out = np.zeros(len(b.coeffs), LD)
    for n in b.leaves():
        deg, dep = int(b.degree[n]), int(b.depth[n])
        cen = ((b.bmin[n] + b.bmax[n]) / np.float32(2.0)).astype(LD)
        h = LD(2.0) ** -(dep + 1)
        q = [cen[a] + x * h for a in range(3)]
        G = g(q[0][:, None, None], q[1][None, :, None], q[2][None, None, :])
        A = RC.legendre(x, deg) * w[None, :] * RC.NL_LD[:deg + 1, dep][:, None]
        T = np.einsum("ai,ijk->ajk", A, G)
        T = np.einsum("bj,ajk->abk", A, T)
        T = np.einsum("ck,abk->abc", A, T)
        idx = R.BIDX[:int(R.COUNT[deg])]
        out[b.start[n]:b.start[n] + len(idx)] = T[idx[:, 0], idx[:, 1], idx[:, 2]] * h ** 3
    return out


@pytest.mark.parametrize("case", ["chain4", "mixed", "chain-deg2", "split-deg3"])
def test_a_global_polynomial_has_no_jump(case):
    """A polynomial of total degree <= the smallest leaf degree, projected exactly into every leaf, is continuous: (M* + D) x = 0.
    M* x vanishes to the entry bounds plus the dropped magnitudes (and the long-double rounding of the product itself and of the
    projection, whose coefficients carry an absolute error of some 2^-60 max |x|)."""
    rng = np.random.default_rng(3)
    if case == "chain-deg2":
        blk, g = deep_chain_block(rng, 5, degrees=(2, 3, 4, 2, 5, 3, 2)), lambda x, y, z: 0.3 + x - 2 * y * z + 0.7 * x * x - z + 0.25 * y * y
    elif case == "split-deg3":
        blk = synthetic_block(rng, [3, 4, 3, 5, 6, 3, 4, 3], depth=2)
        g = lambda x, y, z: 0.1 - y + x * y * z + 2 * z * z * z - 0.5 * x * x * y + 0.3 * y * y
    else:
        blk, g = synthetic_case(case), lambda x, y, z: 0.75 + 0 * (x + y + z)
    ref = RC.reference(blk)
    assert ref.n_numeric > 0 and ref.n_analytic > 0
    x = _project(blk, g)
    xa = np.abs(x).astype(np.float64)
    assert xa.max() > 1e-3
    allowed = ref.matvec(xa, ref.bound + ref.drop) + 2.0 ** -58 * ref.matvec(xa, ref.aval) + 2.0 ** -56 * xa.max() * ref.matvec(np.ones(ref.n), ref.aval)
    got = np.abs(ref.matvec(x)).astype(np.float64)
    assert (got <= allowed).all(), (got / allowed).max()
    assert float(np.abs(ref.matvec(x * (1 + 1e-9 * np.arange(ref.n)))).max()) > allowed.max()    # (the check can fail)


@pytest.mark.parametrize("depth", [1, 2])
def test_constant_leaves_jump_is_difference_squared_times_area(depth):
    """Leaves of degree 0 with values c_k: x^T M* x = sum over touching pairs of (c_1 - c_2)^2 * shared area, the pairs and areas
    found here by brute force over all pairs of boxes -- equal depths (depth 1) and unequal ones (depth 2)."""
    blk = synthetic_block(np.random.default_rng(5), [0] * 8, depth=depth)
    b = R.Block(blk)
    ref = RC.reference(blk)
    lv = b.leaves()
    value = {int(n): LD(b.coeffs[b.start[n]]) * RC.NL_LD[0, b.depth[n]] ** 3 for n in lv}
    want, npairs = LD(0), 0
    for i, j in itertools.combinations([int(n) for n in lv], 2):
        ext = np.minimum(b.bmax[i], b.bmax[j]).astype(LD) - np.maximum(b.bmin[i], b.bmin[j]).astype(LD)
        if (ext == 0).sum() == 1 and (ext >= 0).all():
            npairs += 1
            want += (value[i] - value[j]) ** 2 * np.prod(ext[ext > 0])
    assert npairs == ref.n_pairs == (12 if depth == 1 else 33) and (ref.n_numeric > 0) == (depth == 2)
    got, _ = ref.jump(b.coeffs)
    xa = np.abs(b.coeffs)
    allowed = float((xa * ref.matvec(xa, ref.bound + ref.drop)).sum()) + 2.0 ** -58 * float(want)
    assert want > 0.1 and abs(got - want) <= allowed, (float(got - want), allowed)


def test_reference_matrix_is_symmetric(blocks):
    for name in SYNTHETIC:
        ref = ref_of(name, blocks[name])
        on = ref.must | ref.opt                                                            # the stored entries and their transposes
        tk = (ref.col * ref.n + ref.row)[on]
        t = np.searchsorted(ref.key, tk)
        assert np.array_equal(ref.key[t], tk), name
        assert np.array_equal(ref.must[t], ref.must[on]) and np.array_equal(ref.opt[t], ref.opt[on])
        # (i, j) and (j, i) are evaluated with their factors in the other order: they differ by long-double rounding alone, which
        # LDSLACK takes to be below 2^-10 of the bound
        assert (np.abs(ref.val[t] - ref.val[on]).astype(np.float64) <= 2.0 ** -10 * ref.bound[on]).all(), name
        assert ref.offpattern <= 1e-17 * ref.aval.max(), name


# ------------------------------------------------------------------------------------------------------------ the matrices
def check_matrix(ref, rp, ci, v, st, who):
    ratio, outside, missing = ref.compare(rp, ci, v)
    assert (st["n_pairs"], st["n_pairs_analytic"], st["n_pairs_numeric"]) == (ref.n_pairs, ref.n_analytic, ref.n_numeric), who
    assert outside == 0 and missing == 0, (who, outside, missing)
    assert ratio <= 1, (who, ratio)
    return ratio


@pytest.mark.parametrize("name", SYNTHETIC + ("built",))
def test_oracle_and_host_matrix_within_the_entry_bounds(O, H, blocks, name):
    """ora_continuity_matrix and hpsdf_continuity_matrix against M*: the same pair counts (the reference finds its pairs from the
    boxes, they by NodeProc / FaceProc), the pattern between must and must | optional, every value within its bound."""
    blk = blocks[name]
    ref = ref_of(name, blk)
    assert ref.n_undecided <= 1e-3 * ref.n_contrib, (ref.n_undecided, ref.n_contrib)       # the condition of section 3
    want = {"eight": (12, 0), "mixed": (33, 12), "chain4": (75, 36), "chain10": (201, 108)}.get(name)
    if want:
        assert (ref.n_pairs, ref.n_numeric) == want
    else:
        assert ref.n_numeric > 1000 and ref.n_analytic > 1000
    if name == "mixed":
        assert ref.longest_row == 1303 and ref.n == 4431 and ref.nnz == 523387
    worst = max(check_matrix(ref, *O.Tree.from_block(blk).continuity_matrix(), "oracle"),
                check_matrix(ref, *H.continuity_matrix(blk, 4), "host"))
    assert worst > 0


def _excess(true, mut):
    """The largest |mutant - reference| / bound over the reference's stored entries (an entry the mutant lacks counts as zero)."""
    at = np.minimum(np.searchsorted(mut.key, true.key), len(mut.key) - 1)
    mv = np.where(mut.key[at] == true.key, mut.val[at], LD(0))
    m = true.must
    return float((np.abs(mv[m] - true.val[m]).astype(np.float64) / true.bound[m]).max())


@pytest.mark.parametrize("name", SYNTHETIC)
def test_entry_bounds_reject_the_mutants(blocks, name):
    """Each mutant of the operation leaves the bound in at least one entry of every case it applies to: L(+1) and L(-1) swapped;
    invT of one axis negated; invDist of depth difference d taken as d - 1; scale12 of the coarse leaf's face; NormalisedLengths of
    the other leaf's depth; one fine neighbour of a coarse leaf left out; a Gauss rule one point short.  Those about
    non-conforming faces apply to the trees that have some."""
    true = ref_of(name, blocks[name])
    seen = set()
    for m in RC.MUTANTS:
        if true.n_numeric == 0 and m not in ("face_swap", "gauss_short"):
            continue
        assert _excess(true, RC.reference(blocks[name], mut=m)) > 1, (name, m)
        seen.add(m)
    assert seen == set(RC.MUTANTS) or true.n_numeric == 0


# ------------------------------------------------------------------------------------------------------------ the solves
_XSTAR = {}


def xstar(name, ref, blk):
    k = _key(name, blk)
    if k not in _XSTAR:
        _XSTAR[k] = RC.solve(ref, R.Block(blk).coeffs, RC.strength_of(blk))
    return _XSTAR[k]


# The second, tighter tolerance of the solves: 1e-9 where the drift term of hiprec_continuity section 4 is at least two orders below
# tol ||b|| there, else the smallest power of ten at which it is.  The term is a property of the reference system, not of a solver: it
# is dominated by the first residual's m u |A| |b|, which comes to 0.068 of 1e-9 ||b|| on the mixed tree (rows of 1303 entries) and to
# 0.23 on the chain to depth 10 (entries of 1e5 on the deep leaves), and to at most 6e-3 on the others.  check_solve asserts the
# condition for every solve it sees, at the default tolerance too.
TIGHT_TOL = {"mixed": 1e-8, "chain10": 1e-7}


def tol_of(name, which):
    return 0.0 if which == "default" else TIGHT_TOL.get(name, 1e-9)


def check_solve(ref, blk, out, st, tol, who, star=None):
    """Section 4 of hiprec_continuity for one post-process -> the figures, each as a fraction of what it may be."""
    f = RC.solve_figures(ref, blk, out, st, tol)
    print("%s: residual %.3g of %.3g allowed (stop %.3g, drift %.3g, matrix %.3g), jumps %.3g %.3g of their bounds"
          % (who, f["res"], f["allowed"], f["stop"], f["drift"], f["matrix"], f["jump_before"], f["jump_after"]))
    assert f["drift"] <= 1e-2 * f["stop"], (who, f["drift"], f["stop"])          # negligible at every case and tolerance run
    assert f["res"] <= f["allowed"], (who, f["res"], f["allowed"])
    assert f["jump_before"] <= 1 and f["jump_after"] <= 1, (who, f["jump_before"], f["jump_after"])
    got = {"residual": f["res"] / f["allowed"], "drift": f["drift"] / (1e-2 * f["stop"]), "jump": max(f["jump_before"], f["jump_after"])}
    if star is not None:
        xs, own = star
        err = RC.norm2(f["x"].astype(LD) - xs)
        assert err <= f["err_bound"] + own, (who, err, f["err_bound"])
        got["error"] = err / (f["err_bound"] + own)
    return got


@pytest.mark.parametrize("which", ["default", "tight"])
@pytest.mark.parametrize("name", SYNTHETIC + ("built", "x256"))
def test_host_and_oracle_cg_against_the_true_residual(O, H, blocks, name, which):
    """hpsdf_continuity_post_process on the host and ora_continuity_post_process: the true residual b - A* x in long double obeys
    the stopping rule plus the derived drift (asserted to be below 1e-2 of tol ||b||) and matrix terms, at the default tolerance and at
    TIGHT_TOL; x is within ||r|| / lambda of a long-double LU solve (n <= 4500);
    the statistics' jump energies are x^T M* x within their bounds."""
    blk = blocks[name] if name in blocks else synthetic_case(name)
    tol = tol_of(name, which)
    ref = ref_of(name, blk)
    star = xstar(name, ref, blk) if ref.n <= 4500 else None
    out, st = H.continuity_post_process(blk, tol, 0, 4)
    check_solve(ref, blk, out, st, tol, "host " + name, star)
    assert st["iterations"] > 0 and out[8 + 8 * ref.n:] == blk[8 + 8 * ref.n:]
    t = O.Tree.from_block(blk)
    so = t.continuity_post_process(tol if tol > 0 else 1e-6)
    check_solve(ref, blk, t.to_block(), so, tol if tol > 0 else 1e-6, "oracle " + name, star)


# ||x_k - x_k(long double)|| / ||x_k|| of the ORACLE's CG (ora_continuity_post_process, max_iter = k, tol 1e-30) against the textbook
# Jacobi-PCG of hiprec_continuity.pcg from the same start, measured on the five synthetic cases: at most 1.03e-15 (k = 1), 8.3e-16
# (k = 2), 1.27e-15 (k = 3), 3.83e-15 (k = 5).  Eight times that for another summation order -- far inside the project's 1e-6.
ITERATE_TOL = {1: 8.3e-15, 2: 6.6e-15, 3: 1.1e-14, 5: 3.1e-14}


def check_capped(ref, blk, run, who, star):
    """run(k) -> (block, stats) of a post-process capped at k iterations with tol 1e-30, k in {1, 2, 3, 5}: exactly k iterations;
    the A*-norm of the error x_k - x* below the initial guess's and strictly decreasing in k (what defines CG); and x_k the k-th
    iterate of a long-double Jacobi-PCG from the same start, to ITERATE_TOL.  Returns the largest discrepancy / ITERATE_TOL."""
    c, lam = R.Block(blk).coeffs, RC.strength_of(blk)
    _, want = RC.pcg(ref, c, lam, 5, keep=(0, 1, 2, 3, 5))
    xs = star[0]
    prev = float(ref.energy(want[0] - xs, lam))
    worst = 0.0
    for k in (1, 2, 3, 5):
        out, st = run(k)
        assert st["iterations"] == k, (who, k, st["iterations"])
        x = R.Block(out).coeffs.astype(LD)
        e = float(ref.energy(x - xs, lam))
        assert e < prev, (who, k, e, prev)
        prev = e
        d = RC.norm2(x - want[k]) / RC.norm2(want[k])
        print("%s: iterate %d off the long-double one by %.3g (allowed %.3g), error energy %.6g" % (who, k, d, ITERATE_TOL[k], e))
        assert d <= ITERATE_TOL[k], (who, k, d)
        worst = max(worst, d / ITERATE_TOL[k])
    return worst


@pytest.mark.parametrize("name", SYNTHETIC + ("x256",))
def test_host_capped_runs_are_conjugate_gradient_iterates(O, H, blocks, name):
    """The host solve and the oracle's, capped at 1, 2, 3 and 5 iterations: see check_capped."""
    blk = blocks[name] if name in blocks else synthetic_case(name)
    ref = ref_of(name, blk)
    star = xstar(name, ref, blk)
    check_capped(ref, blk, lambda k: H.continuity_post_process(blk, 1e-30, k, 4), "host " + name, star)

    def oracle(k):
        t = O.Tree.from_block(blk)
        st = t.continuity_post_process(1e-30, k)
        return t.to_block(), st

    check_capped(ref, blk, oracle, "oracle " + name, star)


def test_a_root_that_is_a_leaf_has_nothing_to_solve(H, O):
    """No pairs, an empty matrix; A = lambda I, and CG's first step from x_0 = lambda c lands on c (to the rounding of
    lambda c - lambda^2 c: a few u |c|) with nothing left to iterate."""
    blk = RC.with_strength(root_leaf_block(np.random.default_rng(9), 5), STRENGTH)
    ref = RC.reference(blk)
    assert (ref.n_pairs, ref.nnz, ref.n) == (0, 0, 56)
    rp, ci, v, st = H.continuity_matrix(blk, 2)
    assert st["n_pairs"] == 0 and st["nnz"] == 0 and len(v) == 0 and not rp.any()
    out, sp = H.continuity_post_process(blk)
    c, x = R.Block(blk).coeffs, R.Block(out).coeffs
    assert sp["iterations"] == 0 and sp["jump_before"] == 0 and sp["jump_after"] == 0
    assert (np.abs(x - c) <= 16 * R.U * np.abs(c)).all()
    t = O.Tree.from_block(blk)
    t.continuity_post_process(1e-6)
    assert (np.abs(R.Block(t.to_block()).coeffs - c) <= 16 * R.U * np.abs(c)).all()


def root_leaf_block(rng, degree):
    """A MemoryBlock whose root is a leaf of `degree` over [-0.5, 0.5]^3."""
    node = np.zeros(56, np.uint8)
    node[0:8] = np.array([0xFFFFFFFFFFFFFFFF], np.uint64).view(np.uint8)
    node[8:32] = np.array([-0.5] * 3 + [0.5] * 3, np.float32).view(np.uint8)
    node[40] = degree
    coeffs = rng.standard_normal(int(R.COUNT[degree]))
    cfg = np.zeros(80, np.uint8)
    cfg[40:48] = np.array([1e-10], np.float64).view(np.uint8)
    cfg[48:56] = np.array([1], np.uint64).view(np.uint8)
    cfg[56:80] = np.array([-0.5] * 3 + [0.5] * 3, np.float32).view(np.uint8)
    return (np.array([len(coeffs)], np.uint64).tobytes() + coeffs.tobytes() + np.array([1], np.uint64).tobytes() + node.tobytes()
            + cfg.tobytes())
