"""Fits and builds on the device for the field kinds a fit can sample besides an analytic one -- a mesh (the fused mesh fit, the
sampler and the fits from its sample buffer) and either kind under the tree-CSG wrapper -- against the extended-precision
reference: tests/hiprec.py section 1 ("Data", "Tree CSG") and the build replay of tests/hiprec_build.py.  The cases, the mutants
that show the bounds bite and the oracle's side are in tests/test_hiprec_fields_cpu.py; the long-double caches are shared with it.
The parity tests pin these kernels to the oracle on tiny inputs in the exact mode; these pin every mode to the mathematics, with
the values the oracle's scan gives taken as the data (the anchor test shows the kernels see the same values)."""
import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
import test_hiprec_fields_cpu as T
from conftest import bits
from test_gpu_hiprec import K_MFMA_CELLS, fit_cells_per_group

pytestmark = pytest.mark.gpu

MODES = ("exact", "default", "split", "split_mfma", "fast")
# The largest observed figure / bound of the module, printed as its last line.
WORST = {}
BUILD_WORST = {"leaf rows": 0.0, "job errors": 0.0, "decision margin": np.inf, "total drift / B": 0.0}
_RUNS = {}


@pytest.fixture(scope="module")
def contexts(H, ctx):
    exact = H.Context(0)
    exact.set_fit_mode(H.FIT_EXACT)
    split = H.Context(0)
    split.set_fit_mode(H.FIT_SPLIT)
    split.set_split_min_degree(2)
    fast = H.Context(0)
    fast.set_fast_fit(True)
    yield {"exact": exact, "default": ctx, "split": split, "split_mfma": split, "fast": fast}
    for c in (exact, split, fast):
        c.close()
    print("\nmesh and CSG fields, largest figure / bound: fits " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))
          + "; builds leaf rows %.3g, job errors %.3g, smallest decision margin %.3g bounds, total drift / B %.3g"
          % (BUILD_WORST["leaf rows"], BUILD_WORST["job errors"], BUILD_WORST["decision margin"], BUILD_WORST["total drift / B"]))


# ---------------------------------------------------------------------------------------------------------------- the anchor
def _replay_positions(O, rep, n, rng):
    """n sample positions of the fits a replay made: `n // 100` of its fits, 100 samples of each."""
    keys = list(rep["fits"].cache)
    out = []
    for k in rng.choice(len(keys), n // 100, replace=False):
        box, p, depth, _ = keys[k]
        lo, hi = np.frombuffer(box, np.float32, 3, 0), np.frombuffer(box, np.float32, 3, 12)
        wx, _ = R.sample_axes(*T.BUILD_ROOT, lo, hi, 4 * p + 1)
        i = rng.integers(0, 4 * p + 1, (100, 3))
        out.append(np.stack([wx[a][0, i[:, a]] for a in range(3)], 1))
    return np.concatenate(out)


def test_the_kernels_see_the_values_the_references_are_fed(H, O, ctx, runs):
    """On 20 000 of the replay's sample positions -- float64, as the fits form them -- the device's scan (eval_naive), its
    per-point traversal (eval_lane: the fused mesh fit, a mesh under the wrapper) and the sampler's shared traversal (eval_wave)
    give the oracle's bits at the float32-cast position: the table the references take as exact is the table the kernels read."""
    rep = runs("octa")["free"]
    pts = _replay_positions(O, rep, 20000, np.random.default_rng(77))
    assert pts.shape == (20000, 3) and len(np.unique(pts, axis=0)) > 15000
    want = T.oracle_mesh(O, "octa").mesh.signed_distance(pts.astype(np.float32))[0].astype(np.float64)
    assert (want < 0).any() and (want > 0).any()
    f = H.Field.mesh(ctx, *T.octahedron())
    for name in ("eval_naive", "eval_lane", "eval_wave"):
        got = getattr(f, name)(ctx, pts)
        assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
    f.close()


# ---------------------------------------------------------------------------------------------------------------- fits
def _run_modes(H, O, contexts, monkeypatch, field, p, depth, n, left=False, oracle_cells=None):
    """hpsdf_fit_cells in every mode on one case: all results within the bound; a cell fitted twice (the lattice wraps) the same
    bits; the exact mode the oracle's bits; the split fit's errors the exact kernel's bits; FIT_FAST the exact kernel's bits
    throughout (fitMfmaSupports declines meshes and wrapped fields, so the matrix-core fit must not have run)."""
    nd = T.distinct_cells(depth, n)
    ref, bmin, bmax, root = T.reference(O, field, p, depth, nd, left)
    lattice = np.arange(n) % nd
    refn = {k: v[lattice] for k, v in ref.items()}
    cfg = H.make_config(1e-5, *root)
    got = {}
    for mode in MODES:
        if mode == "split_mfma" and p < 4:
            continue
        hf, keep = T.product_field(H, contexts[mode], field, root, depth)
        if mode == "split_mfma":
            monkeypatch.setenv("HPSDF_LOW_KERNEL", "mfma")
        try:
            c, e = H.fit_cells(contexts[mode], cfg, hf, p, depth, n)
        finally:
            monkeypatch.delenv("HPSDF_LOW_KERNEL", raising=False)
            hf.close()
            for k in keep:
                k.close()
        rc, re = R.fit_ratio(refn, c, e)
        key = mode + ("_left" if left else "")
        WORST[key] = max(WORST.get(key, 0.0), rc, re)
        print("%s p%d d%d n%d %s: coefficients %.3g, errors %.3g of the bound" % (field, p, depth, n, key, rc, re))
        assert rc <= 1 and re <= 1, (mode, field, p, depth, n, rc, re)
        for i in range(nd, n):
            j = int(lattice[i])
            assert np.array_equal(bits(c[i]), bits(c[j])) and bits(e[i:i + 1])[0] == bits(e[j:j + 1])[0], (mode, i, j)
        got[mode] = (c, e)
    c, e = got["exact"]
    cells = sorted({int(lattice[i]) for i in (range(n) if oracle_cells is None else oracle_cells)})
    wc, we = T.oracle_fits(O, field, root, depth, bmin, bmax, p, cells)
    for k, i in enumerate(cells):
        assert np.array_equal(bits(c[i]), bits(wc[k])) and bits(e[i:i + 1])[0] == bits(we[k:k + 1])[0], (field, p, depth, i)
    assert np.array_equal(bits(got["split"][1]), bits(e))
    assert np.array_equal(bits(got["fast"][0]), bits(c)) and np.array_equal(bits(got["fast"][1]), bits(e))
    return got


@pytest.mark.parametrize("case", T.fit_cases(), ids=lambda c: "p%d-d%d-%s-n%d" % c)
def test_cell_fits_within_the_reference_bounds(H, O, contexts, monkeypatch, case):
    """Degrees {2, 3, 5, 8, 11} x depths {0, 1, 4, 8, 10}, every degree meeting every field: two meshes (the fused mesh fit,
    fit_kernel<kFieldMesh>) and union / subtract / intersect over synthetic old trees of degrees 0..12 and depths up to 10, with an
    analytic and a mesh inner (applyCsg and queryPoint<12> inside the fit; with an analytic inner the split fit's lower rows come
    from the samples the wrapped exact kernel leaves).  Counts 1 and 15 are a lone partial 16-cell tile, 16 a full one, 17 and 33
    full tiles and a one-cell tail.  The depth-0 and depth-1 CSG cases fit cells shallower than the old leaves under them: the
    centre node of the odd rule lies on old leaves' faces (tests/test_hiprec_fields_cpu.py shows which leaf the reference takes)."""
    p, depth, field, n = case
    _run_modes(H, O, contexts, monkeypatch, field, p, depth, n)


# One large launch per kind: several fits per workgroup of the term-by-term kernel with a partial last workgroup at degree 3, and
# at degree 11 (one fit per workgroup) 65 cells = four 16-cell tiles and a one-cell tail.  The CSG launches wrap around lattices
# of 64 and 8 cells that are exactly the old trees' leaves (degrees 8..12 and 0..7).
LARGE = (("ico", 3, 4, 601), ("intersect", 3, 2, 601), ("octa", 11, 4, 65), ("subtract", 11, 1, 65))


@pytest.mark.parametrize("field,p,depth,n", LARGE, ids=lambda v: str(v))
def test_large_launches_within_the_reference_bounds(H, O, contexts, monkeypatch, field, p, depth, n):
    g_exact = fit_cells_per_group(p, int(R.COUNT[p]), n)
    g_split = fit_cells_per_group(p, int(R.COUNT[p] - R.COUNT[p - 1]), n)
    assert n % K_MFMA_CELLS != 0
    assert (g_exact > 1 and n % g_exact) or p == 11, (p, n, g_exact)
    assert g_split == 1 or n % g_split, (p, n, g_split)
    _run_modes(H, O, contexts, monkeypatch, field, p, depth, n, oracle_cells=list(range(8)) + list(range(n - 8, n)))


@pytest.fixture
def left_assoc(H, O):
    H.set_reduction_order(1)
    O.set_reduction_order(1)
    yield
    H.set_reduction_order(0)
    O.set_reduction_order(0)


def test_cell_fits_left_associated_within_the_reference_bounds(H, O, contexts, monkeypatch, left_assoc):
    """hpsdf_set_reduction_order(1) under the wrapper: the leftAssoc instantiations, the inner analytic field evaluated in that
    order by the reference too; depth-1 cells over the depth-2 leaves of the old tree (centre nodes on their faces)."""
    _run_modes(H, O, contexts, monkeypatch, "intersect", 5, 1, 17, left=True)


# ---------------------------------------------------------------------------------------------------------------- builds
def _stepwise(H, ctx, O, name):
    """Build.select / jobs / compute / results_host / apply on the GPU under check_round -> (block, stats, Guided.finish's
    observations): a mesh's rounds through the sampler and the fits from its buffer, the union's through the wrapped fit."""
    target, K = T.BUILD_CASES[name]
    f, keep = T.build_product_field(H, ctx, O, name)
    b = H.Build(H.make_config(target, *T.BUILD_ROOT), K, 0, 1)
    g = B.Guided(T.build_spec(O, name), T.BUILD_ROOT, target, K, fits=T.fits_of(O, name))
    while True:
        n = b.select()
        if n == 0:
            break
        jobs = B.job_list(b.jobs(n))
        b.compute(ctx, f)
        headers = b.results_host(ctx).reshape(n, 9)
        g.check_round(jobs, headers)
        b.apply(headers)
    _, counts = b.layout()
    blk = b.assemble([b.pack_host(ctx, counts[0])])
    st = b.stats()
    seen = g.finish(blk, st)
    BUILD_WORST["job errors"] = max(BUILD_WORST["job errors"], seen["job_error"])
    BUILD_WORST["decision margin"] = min(BUILD_WORST["decision margin"], seen["min_margin"])
    BUILD_WORST["total drift / B"] = max(BUILD_WORST["total drift / B"], seen["drift_over_B"])
    f.close()
    for k in keep:
        k.close()
    return blk, st, seen


@pytest.fixture(scope="module")
def runs(H, O, ctx):
    """name -> dict(block, stats, seen of the stepwise run on the default context; free = the free replay of its rounds), made on
    first use and shared by every variant."""
    def get(name):
        if name not in _RUNS:
            blk, st, seen = _stepwise(H, ctx, O, name)
            _RUNS[name] = dict(block=blk, stats=st, seen=seen, free=T.free_replay(O, name, st["rounds"]))
        return _RUNS[name]
    return get


def _rows(O, blk, name, history):
    got = B.check_leaf_rows(blk, T.build_spec(O, name), history, fits=T.fits_of(O, name))
    BUILD_WORST["leaf rows"] = max(BUILD_WORST["leaf rows"], got["worst"])
    assert got["worst"] <= 1, (name, got["worst"])


@pytest.mark.parametrize("name", list(T.BUILD_CASES))
def test_stepwise_build_under_check_round(H, O, runs, name):
    """The stepwise Build with the GPU's fits on a mesh and on a tree-CSG union, every round under check_round: the selection,
    the jobs, all nine errors of every job within their bounds (the alternative's included), every decision the one float64 takes;
    then the block's tree, the statistics, total_error bit for bit from the restated float64 statements and within B of the true
    total, every leaf's rows; and the block is the oracle's."""
    run = runs(name)
    _rows(O, run["block"], name, run["seen"]["history"])
    assert run["seen"]["job_error"] <= 1
    assert run["seen"]["selection_ties"] == 0 and run["seen"]["undecided"] == 0
    assert run["block"] == T.oracle_create(O, name)[0]


VARIANTS = {"octa": ("device", "host", "fused", "exact", "split2", "fast", "ranks2"), "union": ("device", "host", "split2")}


def _one_shot(H, O, contexts, monkeypatch, name, variant):
    target, K = T.BUILD_CASES[name]
    cfg = H.make_config(target, *T.BUILD_ROOT)
    if variant == "ranks2":
        from test_gpu_configs import _create_on_simulated_ranks
        out = _create_on_simulated_ranks(H, 2, cfg, lambda c: T.build_product_field(H, c, O, name)[0], K)
        assert all(blk == out[0][0] for blk, _ in out)
        return out[0]
    monkeypatch.setenv("HPSDF_HOST_FRONTIER", "1" if variant == "host" else "0")
    if variant == "fused":
        monkeypatch.setenv("HPSDF_MESH_FUSED", "1")
    c = contexts[{"split2": "split"}.get(variant, variant if variant in contexts else "default")]
    f, keep = T.build_product_field(H, c, O, name)
    try:
        return H.create_block(c, cfg, f, K)
    finally:
        f.close()
        for k in keep:
            k.close()


def _fits_asked(log):
    """From the replay's job log: (all fits, fits of degree >= 4) the build computes -- a coarse job one degree-2 fit, every other
    job eight child fits of its degree (none at depth 10) and one P fit of degree + 1 (none at degree 11)."""
    total = high = 0
    for (deg, depth, coarse), n in log.items():
        if coarse:
            total += n
            continue
        total += n * ((8 if depth < B.MAX_DEPTH else 0) + (1 if deg < B.MAX_DEGREE - 1 else 0))
        high += n * ((8 if depth < B.MAX_DEPTH and deg >= 4 else 0) + (1 if 3 <= deg < B.MAX_DEGREE - 1 else 0))
    return total, high


@pytest.mark.parametrize("name,variant", [(n, v) for n in VARIANTS for v in VARIANTS[n]])
def test_one_shot_create_against_the_free_replay(H, O, contexts, runs, monkeypatch, name, variant):
    """create_block, one shot, against replay_free grown from long-double errors alone: the tree node by node, rounds / jobs / P /
    H / dropped, every leaf's rows, the stop consistent with the true total, total_error bit for bit the restated float64
    statements.  The mesh: the device frontier (mesh_sample_kernel, then fit_kernel<kFieldSamples> from its buffer), the host
    scheduler, HPSDF_MESH_FUSED=1 (fit_kernel<kFieldMesh>), the exact mode, the split from degree 2 (lower rows by fit_low.hip from
    the sampler's buffer), FIT_FAST (degree >= 4 on the matrix cores from that buffer; its total within B of the true one) and 2
    simulated ranks.  The union: device frontier, host scheduler, split from degree 2.  At this target no node of degree 4 is
    selected again, so the fits of degree >= 4 are the P fits of degree-3 nodes: the statistics say the build was the sampled one in
    the mode asked for and computed every fit the replay's job log counts, at least 16 of them of degree >= 4."""
    target, K = T.BUILD_CASES[name]
    run = runs(name)
    rep, seen = run["free"], run["seen"]
    blk, st = _one_shot(H, O, contexts, monkeypatch, name, variant)
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0
    assert st["rounds"] == run["stats"]["rounds"]
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"]
    assert st["device_frontier"] == (0 if variant in ("host", "fused") else 1)
    _rows(O, blk, name, rep["history"])
    total, high = _fits_asked(rep["job_log"])
    if variant != "ranks2":                                    # (a rank counts its own share)
        assert st["fits"] == total, (st["fits"], total)
    if variant == "fast":
        drift = float(abs(R.LD(st["total_error"]) - rep["true_total"]))
        assert drift <= rep["B"] + rep["true_bound"], (drift, rep["B"])
    else:
        assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes(), (st["total_error"], seen["f64_total"])
    if variant == "split2":
        assert st["fit_mode"] == H.FIT_SPLIT and st["split_fits"] > 0
    if variant == "fast":
        assert st["fit_mode"] == H.FIT_FAST
    if name == "octa" and variant in ("split2", "fast"):
        assert high >= 16 and T.degree4_fits(rep["history"]) >= 16, high
