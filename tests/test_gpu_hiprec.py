"""Cell fits and Query of the product against the extended-precision reference (tests/hiprec.py), in every fit mode, at
degrees 2..11, depths {0, 1, 4, 8, 10}, on three roots and at the tails of the fit kernels' tilings.  The parity tests pin the
kernels to the oracle bit for bit; these pin them -- and, through the exact mode, the oracle -- to the mathematics."""
import numpy as np
import pytest

import hiprec as R
from conftest import bits
from test_hiprec_cpu import ROOTS, query_blocks

pytestmark = pytest.mark.gpu

DEPTHS = (0, 1, 4, 8, 10)
COUNTS = (1, 15, 16, 17, 33)
MODES = ("exact", "default", "split", "split_mfma", "fast")
# The largest observed |kernel - reference| / bound per mode, printed at the end of the module (the slack the bounds leave).
WORST = {}


# ---------------------------------------------------------------------------------------------------------------- shapes
# Restated from csrc/launch.hpp, csrc/fit.hip (fitShape) and csrc/fit_low.hip (LowShape) so that the counts below are
# chosen from the kernels' tilings, not guessed.
K_FIT_THREADS, K_FIT_MAX_LDS, K_MFMA_CELLS = 256, 60 * 1024, 16


def _fit_lds(p, g, planes):
    nq = 4 * p + 1
    return ((p + 1) * nq + 2 * nq + 8 * g + g * planes * nq * nq) * 8


def fit_cells_per_group(p, nrows, count):
    """fitShape(degree, nrows, count, false).cells: the fits one workgroup of the term-by-term kernel carries."""
    slots = 1 if nrows > K_FIT_THREADS else K_FIT_THREADS // nrows
    gmax = slots
    while gmax > 1 and _fit_lds(p, gmax, 1) > K_FIT_MAX_LDS:
        gmax -= 1
    g = min(gmax, max(1, (count + 511) // 512))
    if p == 2:
        g = min(min(gmax, 16), max(1, (count + 1023) // 1024 if count <= 4096 else (count + 511) // 512))
    return g


def low_passes(p):
    """LowShape<p>: (PASSES, AG) of the split kernel's stage 1."""
    nq = 4 * p + 1
    budget = 52 * 1024 - (p * nq + p * (p + 1) // 2 * nq) * 8
    agmax = max(1, budget // (nq * nq * 8))
    passes = (p + agmax - 1) // agmax
    return passes, (p + passes - 1) // passes


def _ncoef(p):
    return int(R.COUNT[p])


# Large launches: a few thousand cells at low degree, a few hundred at degree 11.  Each count leaves a partial last workgroup of
# the term-by-term kernel (count % fitShape.cells != 0, asserted in the test) and a partial 16-cell tile of the matrix-core kernels.
LARGE = ((2, 4, 3001), (3, 8, 2999), (4, 8, 2066), (11, 4, 257))


def _cases():
    """Every degree meets every depth; each case runs in every mode, so every degree meets every mode.  Roots, counts and fields
    rotate with the case."""
    out = []
    fields = ("sphere", "box", "crease", "carve", "plane")
    for p in range(2, 12):
        for di, d in enumerate(DEPTHS):
            out.append((p, d, list(ROOTS)[(p + di) % 3], COUNTS[(p + 2 * di) % 5], fields[(p + di) % 5]))
    return out


def _reference(spec, root, depth, p, n, left=False):
    bmin, bmax = R.lattice_cells(depth, n)
    parts = []
    step = max(1, 2 ** 21 // (4 * p + 1) ** 3)           # cells per reference batch (bounded memory)
    for i in range(0, n, step):
        parts.append(R.fit_reference(spec, *ROOTS[root], bmin[i:i + step], bmax[i:i + step], p, depth, left))
    return {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}, bmin, bmax


@pytest.fixture(scope="module")
def contexts(H, ctx):
    exact = H.Context(0)
    exact.set_fit_mode(H.FIT_EXACT)
    split = H.Context(0)
    split.set_split_min_degree(2)
    fast = H.Context(0)
    fast.set_fast_fit(True)
    made = {"exact": exact, "default": ctx, "split": split, "split_mfma": split, "fast": fast}
    yield made
    for c in (exact, split, fast):
        c.close()
    if WORST:
        print("\nlargest |kernel - reference| / bound per mode: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _run_modes(H, O, contexts, monkeypatch, p, depth, root, n, field, left=False, oracle_cells=None):
    rmin, rmax = ROOTS[root]
    spec = R.corner_fields(rmin, rmax, depth)[field]
    ref, bmin, bmax = _reference(spec, root, depth, p, n, left)
    cfg = H.make_config(1e-5, rmin, rmax)
    hf = H.Field.analytic(spec)
    lattice = np.arange(n) % (1 << (3 * depth))
    got = {}
    for mode in MODES:
        if mode == "split_mfma" and p < 4:
            continue
        if mode == "split_mfma":
            monkeypatch.setenv("HPSDF_LOW_KERNEL", "mfma")
        try:
            c, e = H.fit_cells(contexts[mode], cfg, hf, p, depth, n)
        finally:
            monkeypatch.delenv("HPSDF_LOW_KERNEL", raising=False)
        rc, re = R.fit_ratio(ref, c, e)
        key = mode + ("_left" if left else "")
        WORST[key] = max(WORST.get(key, 0.0), rc, re)
        assert rc <= 1 and re <= 1, (mode, p, depth, root, n, field, rc, re)
        # a cell fitted twice (the lattice wraps) gets the same bits in every tile and workgroup
        first = {}
        for i, l in enumerate(lattice):
            j = first.setdefault(int(l), i)
            if j != i:
                assert np.array_equal(bits(c[i]), bits(c[j])) and bits(e[i:i + 1])[0] == bits(e[j:j + 1])[0], (mode, i, j)
        got[mode] = (c, e)
    # the exact mode is the oracle, bit for bit, at these depths, roots and fields
    ocfg, of = O.default_config(1e-5, rmin, rmax), O.AnalyticField(spec)
    c, e = got["exact"]
    for i in (range(n) if oracle_cells is None else oracle_cells):
        wc, we = O.fit_polynomial(of, ocfg, bmin[i], bmax[i], p, depth)
        assert np.array_equal(bits(c[i]), bits(wc)) and bits(e[i:i + 1])[0] == bits(np.array([we]))[0], (p, depth, root, i)
    # the error of a split fit is the exact kernel's (its top rows are); the default context is the exact kernel below degree 6
    assert np.array_equal(bits(got["split"][1]), bits(e))
    if p < 6:
        assert np.array_equal(bits(got["default"][0]), bits(c))
    return got


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "p%d-d%d-%s-n%d-%s" % c)
def test_cell_fits_within_the_reference_bounds(H, O, contexts, monkeypatch, case):
    """Every coefficient and every error of hpsdf_fit_cells, in FIT_EXACT, the default context, FIT_SPLIT from degree 2 (lower rows
    by fit_low.hip, and with HPSDF_LOW_KERNEL=mfma by the matrix cores) and FIT_FAST, within the derived bound of the reference;
    the exact mode also the oracle's bits.  Counts 1 and 15 are a lone partial 16-cell tile of the matrix-core kernels, 16 a full
    one, 17 and 33 full tiles and a one-cell tail; depth 0 (and depth 1 at 33 cells) fits one cell again and again."""
    p, depth, root, n, field = case
    _run_modes(H, O, contexts, monkeypatch, p, depth, root, n, field)


@pytest.mark.parametrize("p,depth,n", LARGE, ids=lambda v: str(v))
def test_large_launches_within_the_reference_bounds(H, O, contexts, monkeypatch, p, depth, n):
    """A few thousand cells at low degree, a few hundred at degree 11: several fits per workgroup with a partial last workgroup,
    a partial last 16-cell tile, and (degree 11) the split kernel's eleven stage-1 passes over the samples."""
    g_exact = fit_cells_per_group(p, _ncoef(p), n)
    g_split = fit_cells_per_group(p, _ncoef(p) - _ncoef(p - 1), n)
    assert n % K_MFMA_CELLS != 0
    assert (g_exact > 1 and n % g_exact) or p == 11, (p, n, g_exact)
    assert g_split == 1 or n % g_split, (p, n, g_split)
    root = list(ROOTS)[p % 3]
    _run_modes(H, O, contexts, monkeypatch, p, depth, root, n, ("sphere", "crease", "carve", "box")[p % 4],
               oracle_cells=list(range(8)) + list(range(n - 8, n)))


def test_split_passes_are_exercised():
    """The degrees whose split kernel runs stage 1 in several passes (LowShape::PASSES > 1), one of them with a partial last pass,
    are all in the case grid above."""
    multi = [p for p in range(2, 12) if low_passes(p)[0] > 1]
    assert multi == [7, 8, 9, 10, 11]
    assert [p for p in multi if p % low_passes(p)[1]] == [7]
    assert {c[0] for c in _cases()} >= set(multi)


@pytest.fixture
def left_assoc(H, O):
    H.set_reduction_order(1)
    O.set_reduction_order(1)
    yield
    H.set_reduction_order(0)
    O.set_reduction_order(0)


@pytest.mark.parametrize("case", [(2, 4, "cube", 17, "carve"), (5, 1, "aniso", 33, "crease"), (8, 8, "unit", 16, "sphere"),
                                  (11, 10, "cube", 15, "box")], ids=lambda c: "p%d-d%d-%s-n%d-%s" % c)
def test_cell_fits_left_associated_within_the_reference_bounds(H, O, contexts, monkeypatch, left_assoc, case):
    """hpsdf_set_reduction_order(1): the leftAssoc instantiations of every fit kernel, within the same bounds (the reference
    evaluates its fields in the same order), and the exact mode still the oracle's bits under the same switch."""
    p, depth, root, n, field = case
    _run_modes(H, O, contexts, monkeypatch, p, depth, root, n, field, left=True)


# ---------------------------------------------------------------------------------------------------------------- query
def _query_check(H, ctx, name, blk, rng):
    tree = H.DeviceTree(ctx, blk)
    pts = R.points_in_leaves(blk, rng, 1200)
    ref = R.fapprox_reference(blk, pts, gradient=True)
    order = np.argsort(ref["leaf"], kind="stable")       # a cell-sorted set: the ordered-input path
    for label, idx in (("few", np.arange(24)), ("general", np.arange(len(pts))), ("sorted", order)):
        v = tree.query(pts[idx])
        vg, g = tree.query_with_gradient(pts[idx])
        rv = (np.abs(v.astype(R.LD) - ref["f"][idx]).astype(np.float64) / ref["f_bound"][idx]).max()
        rvg = (np.abs(vg.astype(R.LD) - ref["f"][idx]).astype(np.float64) / ref["f_bound"][idx]).max()
        rg = (np.abs(g.astype(R.LD) - ref["g"][idx]).astype(np.float64) / ref["g_bound"][idx]).max()
        WORST["query"] = max(WORST.get("query", 0.0), rv, rvg)
        WORST["gradient"] = max(WORST.get("gradient", 0.0), rg)
        assert rv <= 1 and rvg <= 1 and rg <= 1, (name, label, rv, rvg, rg)


def test_query_within_the_reference_bounds(H, ctx, contexts):
    """DeviceTree.query and query_with_gradient on synthetic blocks (degrees 0..12, depths 1..10, two roots) at points strictly
    inside leaves: 24 points (answered on the host), 1200 random points and the same points sorted by cell."""
    rng = np.random.default_rng(21)
    for name, blk in query_blocks(rng):
        _query_check(H, ctx, name, blk, rng)


@pytest.mark.parametrize("root", list(ROOTS))
def test_built_tree_query_within_the_reference_bounds(H, ctx, contexts, root):
    """One tree built on the device per root (a sphere's surface near the root's corner), queried within the bounds."""
    rmin, rmax = ROOTS[root]
    spec = R.corner_fields(rmin, rmax, 2)["crease"]
    blk, _ = H.create_block(ctx, H.make_config(1e-6, rmin, rmax), H.Field.analytic(spec), 1024)
    _query_check(H, ctx, "built-" + root, blk, np.random.default_rng(31))
