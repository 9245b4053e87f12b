"""The build loop against its extended-precision replay (tests/hiprec_build.py) on the CPU: the oracle's one-shot Create against
the free replay, the product's host scheduler (fed the oracle's numerics) under check_round every round, the stop rule's float64
drift as a test, and mutants of the replay that the checks reject."""
import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
from test_hiprec_cpu import ROOTS

# name: (root, corner_fields' depth, field, target, K), chosen by running this module.  A free case is far from every tie -- a
# condition on the inputs: the oracle's own build meets zero undecided decisions and selections -- and runs through replay_free
# and check_round; a tie case has reference errors at the K-th place closer than their bounds and runs under check_round only.
#   aniso-sphere   2 rounds, 232 P and 24 H past round 0: the quick one, carries the mutants
#   aniso-sphere9  141 rounds of 16: a leaf of degree 6, four P-appends on one leaf, an H at depth 6
#   unit-sphere9   188 rounds of 16: target 1e-10, the float64 total ends at -4.3e-11 with the true total at 1.0e-8
#   cube-allK      K = 8192 above the 4096 queued entries: round 1 takes the whole queue
#   unit-carve     4 rounds, ties at the K-th place in two of them;  cube-crease: the first ties of the 3e-7 build
FREE_CASES = {
    "aniso-sphere": ("aniso", 2, "sphere", 1e-5, 256),
    "aniso-sphere9": ("aniso", 9, "sphere", 1e-9, 16),
    "unit-sphere9": ("unit", 9, "sphere", 1e-10, 16),
    "cube-allK": ("cube", 2, "sphere", 1e-6, 8192),
}
TIE_CASES = {
    "unit-carve": ("unit", 2, "carve", 1e-7, 256),
    "cube-crease": ("cube", 2, "crease", 3e-6, 64),
}
CASES = dict(FREE_CASES, **TIE_CASES)
SEEN = {}
_CACHE = {}


def case_spec(name):
    root, depth, field, target, K = CASES[name]
    return R.corner_fields(*ROOTS[root], depth)[field], ROOTS[root], target, K


def fits_of(name):
    """One cache of long-double fits per case, shared by every test of this module (and of the GPU module)."""
    if ("fits", name) not in _CACHE:
        spec, root, _, _ = case_spec(name)
        _CACHE["fits", name] = B.Fits(spec, root)
    return _CACHE["fits", name]


def oracle_create(O, name):
    if ("create", name) not in _CACHE:
        spec, root, target, K = case_spec(name)
        t = O.Tree.create(O.default_config(target, *root), O.AnalyticField(spec), K)
        _CACHE["create", name] = (t.to_block(), t.stats)
    return _CACHE["create", name]


def free_replay(name, rounds):
    if ("free", name) not in _CACHE:
        spec, root, target, K = case_spec(name)
        _CACHE["free", name] = B.replay_free(spec, root, target, K, rounds, fits=fits_of(name))
    return _CACHE["free", name]


def run_guided(H, O, name, mutant=None, K=None):
    """test_product_cpu.run_injected's loop on one rank -- the product's host scheduler, the oracle's job numerics -- under
    check_round every round -> (block, stats, what Guided.finish observed, the rounds' (jobs, headers))."""
    spec, root, target, K0 = case_spec(name)
    cfg, ocfg, f = H.make_config(target, *root), O.default_config(target, *root), O.AnalyticField(spec)
    b = H.Build(cfg, K0, 0, 1)
    g = B.Guided(spec, root, target, K0 if K is None else K, mutant=mutant, fits=fits_of(name))
    rounds = []
    while True:
        n = b.select()
        if n == 0:
            break
        jobs = b.jobs(n)
        headers = np.zeros((n, 9))
        for j in range(n):
            jb = jobs[j]
            res, pc, hc = O.job(f, ocfg, tuple(jb.aabb_min), tuple(jb.aabb_max), jb.depth, jb.degree, jb.err,
                                None if jb.coarse else np.zeros(O.NCOEF[jb.degree]))
            headers[j, 0] = res.p_err
            headers[j, 1:] = list(res.h_err)
            b.inject(j, pc, hc.reshape(-1))
        rounds.append((B.job_list(jobs), headers.copy()))
        g.check_round(*rounds[-1])
        b.apply(headers)
    _, counts = b.layout()
    blk = b.assemble([b.pack_host(None, counts[0])])
    st = b.stats()
    return blk, st, g.finish(blk, st), rounds


def guided(H, O, name):
    if ("guided", name) not in _CACHE:
        _CACHE["guided", name] = run_guided(H, O, name)
    return _CACHE["guided", name]


def test_coarse_tree_is_the_reference_walk():
    """4681 nodes in creation order: every node's children are consecutive, a node's children come after it, the 4096 queued
    nodes are the depth-4 ones in index order, and the boxes tile [-0.5, 0.5]^3 with exact dyadic faces."""
    t, queued = B.coarse_tree()
    a = t.arrays()
    assert len(a["child"]) == 4681 and len(queued) == 4096 and queued == sorted(queued)
    assert [int((a["depth"] == d).sum()) for d in range(5)] == [1, 8, 64, 512, 4096]
    assert (a["depth"][queued] == 4).all() and (a["child"][queued] == -1).all()
    inner = np.nonzero(a["child"] >= 0)[0]
    assert (a["child"][inner] > inner).all() and sorted(a["child"][inner]) == list(range(1, 4681, 8))
    assert a["child"][1] == 9 and a["child"][9] == 17 and a["child"][17] == 25 and queued[:64] == list(range(25, 89)) and queued[64] == 97
    ext = a["bmax"] - a["bmin"]
    assert np.array_equal(ext, np.float32(1.0) / np.float32(2.0) ** a["depth"][:, None] * np.ones((1, 3), np.float32))
    vol = (ext[queued].astype(np.float64).prod(1)).sum()
    assert vol == 1.0


@pytest.mark.parametrize("name", list(FREE_CASES))
def test_oracle_create_equals_the_free_replay(O, name):
    """Tree.create of the oracle, one shot, against replay_free: childIdx, degree, depth and the boxes of every node; rounds, jobs,
    P (round 0's 4096 included), H and dropped; every leaf's rows against the fits that formed them (the replay's history says
    which); zero undecided decisions and selections; the stop consistent with the true total."""
    spec, root, target, K = case_spec(name)
    blk, st = oracle_create(O, name)
    rep = free_replay(name, st["rounds"])
    print("\n%s: rounds %d, jobs past round 0 %d, P %d, H %d, max degree %d, max depth %d, min margin %.3g bounds, fits %d"
          % (name, st["rounds"], st["jobs"] - 4096, st["p_refines"] - 4096, st["h_refines"], rep["degree"][rep["degree"] < 13].max(),
             rep["depth"].max(), rep["min_margin"], rep["fits"].computed))
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0, (rep["undecided_decisions"], rep["undecided_selections"])
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"], (float(rep["true_total"]), rep["true_bound"], rep["B"], target)
    rows = B.check_leaf_rows(blk, spec, rep["history"], fits=fits_of(name))
    print("%s: leaf rows %.3g of the bound, longest chain of P-appends %d" % (name, rows["worst"], rows["chain"]))
    assert rows["worst"] <= 1
    SEEN[name] = dict(max_degree=int(rep["degree"][rep["degree"] < 13].max()), chain=rows["chain"],
                      h_depth=int(rep["depth"][rep["degree"] == 13].max()))


@pytest.mark.parametrize("name", list(CASES))
def test_host_scheduler_under_check_round(H, O, name):
    """The product's host scheduler (Build.select / jobs / inject / apply) with the oracle's job numerics, every round under
    check_round -- the selection within the bounds of the K-th error, the jobs in node order with the boxes, degrees and queued
    errors the replay holds, each live error within its bound, every decided decision the one float64 takes -- then the
    assembled block's tree, the statistics, total_error bit for bit from the restated statements and within B of the true
    total, and every leaf's rows.  The tie cases have exact ties at the K-th place; the replay adopts the product's pick."""
    spec, root, target, K = case_spec(name)
    blk, st, seen, _ = guided(H, O, name)
    print("\n%s: rounds %d, job errors %.3g of the bound, smallest decision margin %.3g bounds, undecided %d, ties at the K-th place %d, "
          "rounds below K entries %d, total drift %.3g of B (B %.3g)" % (name, st["rounds"], seen["job_error"], seen["min_margin"],
                                                                        seen["undecided"], seen["selection_ties"], seen["small_rounds"],
                                                                        seen["drift_over_B"], seen["B"]))
    rows = B.check_leaf_rows(blk, spec, seen["history"], fits=fits_of(name))
    print("%s: leaf rows %.3g of the bound" % (name, rows["worst"]))
    assert rows["worst"] <= 1 and seen["job_error"] <= 1
    if name in TIE_CASES:
        assert seen["selection_ties"] > 0
    if name in FREE_CASES:
        assert blk == oracle_create(O, name)[0]
    SEEN[name + "/guided"] = seen


def test_cases_reach_what_they_are_for(H, O):
    """Between them: a leaf of degree >= 6, a chain of three P-appends on one leaf, an H below depth 6, a round with fewer than K
    queued entries."""
    for name in FREE_CASES:
        if name not in SEEN:
            test_oracle_create_equals_the_free_replay(O, name)
    for name in CASES:
        if name + "/guided" not in SEEN:
            test_host_scheduler_under_check_round(H, O, name)
    free = [SEEN[n] for n in FREE_CASES]
    assert max(s["max_degree"] for s in free) >= 6
    assert max(s["chain"] for s in free) >= 3
    assert max(s["h_depth"] for s in free) >= 6
    assert sum(SEEN[n + "/guided"]["small_rounds"] for n in CASES) > 0


def test_block_alone_tells_which_fit_formed_each_row(O):
    """check_leaf_rows without a history: for a sample of leaves of a built block some p0 in 2..p explains the rows, and it is
    the replay's.  (A leaf never P-refined since its from-scratch fit has p0 = p; a chain shows as p0 < p.)"""
    name = "aniso-sphere9"
    spec, root, target, K = case_spec(name)
    blk, st = oracle_create(O, name)
    rep = free_replay(name, st["rounds"])
    b = R.Block(blk)
    lv = b.leaves()
    deep = lv[np.argsort(-(b.degree[lv] * 16 + b.depth[lv]), kind="stable")[:24]]
    got = B.check_leaf_rows(blk, spec, None, fits=fits_of(name), leaves=deep)
    assert got["worst"] <= 1
    assert {n: rep["history"][n][0] for n in got["p0"]} == got["p0"]
    assert got["chain"] >= 1


def test_stop_rule_is_governed_by_float64_drift(H, O):
    """The finding as a test: a build with target <= 1e-10 stops with the float64 total BELOW the target
    while the true sum of its leaves' errors is ABOVE it.  The float64 total is the restated statements' bit for bit
    (Guided.finish asserts it); its distance from the true total is within B."""
    name = "unit-sphere9"
    spec, root, target, K = case_spec(name)
    assert target <= 1e-10
    blk, st, seen, _ = guided(H, O, name)
    print("\n%s: float64 total %.3e, true total %.3e +- %.1e, target %.0e, drift %.3g = %.3g of B (%.3g)"
          % (name, seen["f64_total"], float(seen["true_total"]), seen["true_bound"], target, seen["drift"], seen["drift_over_B"], seen["B"]))
    assert st["total_error"] == seen["f64_total"] < target
    assert float(seen["true_total"]) - seen["true_bound"] > target
    assert seen["drift"] <= seen["B"]
    assert oracle_create(O, name)[1]["total_error"] == st["total_error"]


# ---------------------------------------------------------------------------------------------------------------- mutants
MUTANT_CASE = "aniso-sphere"


def _free_differs(O, name, **kw):
    spec, root, target, K = case_spec(name)
    blk, st = oracle_create(O, name)
    rep = B.replay_free(spec, root, target, kw.pop("K", K), st["rounds"], fits=fits_of(name), **kw)
    try:
        B.same_tree(blk, rep)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", ["K+1", "K-1"] + list(B.SCHEDULE_MUTANTS))
def test_mutants_of_the_replay_are_caught(H, O, mutant):
    """Each mutant of the replay -- K + 1, K - 1, the two divisors swapped, the factor 8 dropped from either improvement, the mean
    child error for the max, children fitted at degree + 1, child errors normalised at the parent's depth, results applied in
    descending node order -- grows another tree than the oracle's in the free replay, AND (all but the application order, which the
    guided form takes from the product) fails check_round on the host scheduler's rounds.  A check loose enough to admit one of
    them would fail here."""
    name = MUTANT_CASE
    _, _, _, K = case_spec(name)
    kw = {"K": K + 1} if mutant == "K+1" else {"K": K - 1} if mutant == "K-1" else {"mutant": mutant}
    assert _free_differs(O, name, **kw), mutant
    if mutant == "apply_desc":
        return
    rounds = guided(H, O, name)[3]
    spec, root, target, _ = case_spec(name)
    g = B.Guided(spec, root, target, kw.get("K", K), mutant=kw.get("mutant"), fits=fits_of(name))
    with pytest.raises(AssertionError):
        for jobs, headers in rounds:
            g.check_round(jobs, headers)


def test_final_degree_rows_mutant_is_caught(O):
    """check_leaf_rows with every row taken from the fit of the leaf's final degree -- the naive reading -- leaves the bound by
    orders of magnitude where a P-appended leaf holds the feature: rows below COUNT[p0] were formed with the rule of order
    4 p0 + 1, not 4p + 1.  (Far from the feature the field is analytic and both rules are exact to rounding: unit-sphere9 and
    cube-allK cannot tell, and are not asked to.)"""
    for name in ("aniso-sphere", "aniso-sphere9"):
        spec, root, target, K = case_spec(name)
        blk, st = oracle_create(O, name)
        rep = free_replay(name, st["rounds"])
        chained = [n for n, (p0, app) in rep["history"].items() if len(app) >= 1]
        assert chained
        got = B.check_leaf_rows(blk, spec, rep["history"], fits=fits_of(name), leaves=chained, final_fit=True)
        print("\n%s: rows from the final-degree fit are %.3g bounds off" % (name, got["worst"]))
        assert got["worst"] > 1, (name, got["worst"])
