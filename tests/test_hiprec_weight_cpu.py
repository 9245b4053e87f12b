"""Nearness-weighted builds against the extended-precision replay (tests/hiprec_build.py with tests/hiprec_weight.py) on the CPU:
the restated sampler against its own properties and the oracle's points, the oracle's mean and weight piecewise against the
long-double ones, the oracle's weighted one-shot Create against the free replay, the product's host scheduler (fed the oracle's
numerics) under check_round every round, and mutants of the weighting that the checks reject."""
import ctypes as C

import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
import hiprec_weight as W
import test_hiprec_build_cpu as U
from test_hiprec_cpu import ROOTS

# name: (root, corner_fields' depth, field, target, K, (weighting type, strength)), chosen by running this module: roots and fields
# of test_hiprec_build_cpu.CASES, so the long-double fits of a cell are shared with them.  All are free cases: the oracle's own build
# meets zero undecided decisions and selections and no fit excluded as undecided by construction.
#   cube-poly3         Polynomial 3 (the reference's unit test), root of width 5.25: the far coarse cells have m > sqrt 3 and weight
#                      0 exactly.  2 rounds of 64 past round 0, six H at depth 4.  The quick one, carries most mutants.
#   cube-allK-poly2.5  a fractional strength on the same root: the far cells take the NaN branch (weight 1).  K = 8192 above the
#                      4096 queued entries: round 1 takes the whole queue.
#   aniso-exp3         Exponential 3 (the reference's benchmark): 2 rounds of 256, 24 H at depth 4, P arrays of degree 3 and 4.
#   aniso9-exp3        21 rounds of 64: P arrays up to degree 7 that carry up to four appends, H down to depth 6.
CASES = {
    "cube-poly3": ("cube", 2, "sphere", 1e-7, 64, (W.POLYNOMIAL, 3.0)),
    "cube-allK-poly2.5": ("cube", 2, "sphere", 1e-6, 8192, (W.POLYNOMIAL, 2.5)),
    "aniso-exp3": ("aniso", 2, "sphere", 1e-6, 256, (W.EXPONENTIAL, 3.0)),
    "aniso9-exp3": ("aniso", 9, "sphere", 1e-9, 64, (W.EXPONENTIAL, 3.0)),
}
SEEN = {}
_CACHE = {}


def case_spec(name):
    root, depth, field, target, K, weighting = CASES[name]
    return R.corner_fields(*ROOTS[root], depth)[field], ROOTS[root], target, K, weighting


def fits_of(name):
    """The unweighted case's cache of long-double fits where one has this root and field, else one of its own."""
    same = [n for n, c in U.CASES.items() if c[:3] == CASES[name][:3]]
    if same:
        return U.fits_of(same[0])
    if ("fits", name) not in _CACHE:
        spec, root = case_spec(name)[:2]
        _CACHE["fits", name] = B.Fits(spec, root)
    return _CACHE["fits", name]


def weighting_of(name):
    """One cache of long-double weights per case, shared by every test of this module (and of the GPU module)."""
    if ("weighting", name) not in _CACHE:
        _CACHE["weighting", name] = W.Weighting(*CASES[name][5])
    return _CACHE["weighting", name]


def configs(H, O, name):
    spec, root, target, K, (wtype, strength) = case_spec(name)
    ocfg = cfg = None
    if O is not None:
        ocfg = O.default_config(target, *root)
        ocfg.weighting_type, ocfg.weighting_strength = wtype, strength
    if H is not None:
        cfg = H.make_config(target, *root)
        cfg.nearnessWeighting_type, cfg.nearnessWeighting_strength = wtype, strength
    return cfg, ocfg


def oracle_create(O, name):
    if ("create", name) not in _CACHE:
        spec, root, target, K, _ = case_spec(name)
        t = O.Tree.create(configs(None, O, name)[1], O.AnalyticField(spec), K)
        _CACHE["create", name] = (t.to_block(), t.stats)
    return _CACHE["create", name]


def free_replay(name, rounds):
    if ("free", name) not in _CACHE:
        spec, root, target, K, _ = case_spec(name)
        _CACHE["free", name] = B.replay_free(spec, root, target, K, rounds, fits=fits_of(name), weighting=weighting_of(name))
    return _CACHE["free", name]


def run_guided(H, O, name):
    """test_hiprec_build_cpu.run_guided for a weighted build: an incremental weighted fit starts from the node's stored rows
    (Octree.cpp:847), which the scheduler hands out -> (block, stats, what Guided.finish observed, the rounds' (jobs, headers),
    every fit array of the build as (bmin, bmax, depth, degree, float64 coefficients))."""
    spec, root, target, K, _ = case_spec(name)
    (cfg, ocfg), f = configs(H, O, name), O.AnalyticField(spec)
    b = H.Build(cfg, K, 0, 1)
    g = B.Guided(spec, root, target, K, fits=fits_of(name), weighting=weighting_of(name))
    rounds, arrays = [], []
    while True:
        n = b.select()
        if n == 0:
            break
        jobs = b.jobs(n)
        headers = np.zeros((n, 9))
        for j in range(n):
            jb = jobs[j]
            lo, hi = np.array(jb.aabb_min[:], np.float32), np.array(jb.aabb_max[:], np.float32)
            res, pc, hc = O.job(f, ocfg, tuple(jb.aabb_min), tuple(jb.aabb_max), jb.depth, jb.degree, jb.err,
                                None if jb.coarse else b.node_rows(None, jb.node_idx))
            headers[j, 0] = res.p_err
            headers[j, 1:] = list(res.h_err)
            b.inject(j, pc, hc.reshape(-1))
            arrays.append((lo, hi, int(jb.depth), 2 if jb.coarse else jb.degree + 1, pc.copy()))
            if not jb.coarse:
                arrays += [B.corner_aabb(lo, hi, i) + (jb.depth + 1, int(jb.degree), hc[i].copy()) for i in range(8)]
        rounds.append((B.job_list(jobs), headers.copy()))
        g.check_round(*rounds[-1])
        b.apply(headers)
    _, counts = b.layout()
    blk = b.assemble([b.pack_host(None, counts[0])])
    st = b.stats()
    return blk, st, g.finish(blk, st), rounds, arrays


def guided(H, O, name):
    if ("guided", name) not in _CACHE:
        _CACHE["guided", name] = run_guided(H, O, name)
    return _CACHE["guided", name]


def _ora_weight_api(O):
    L = O.lib()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.ora_weight_key.restype, L.ora_weight_key.argtypes = C.c_uint64, [fp, C.c_int, C.c_int]
    L.ora_weight_point.restype, L.ora_weight_point.argtypes = None, [fp, fp, C.c_int, C.c_int, C.c_uint64, dp]
    L.ora_weight_mean.restype, L.ora_weight_mean.argtypes = C.c_double, [dp, C.c_int, fp, fp, C.c_int]
    L.ora_weight_from_mean.restype, L.ora_weight_from_mean.argtypes = C.c_double, [C.c_int, C.c_double, C.c_double]
    return L


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


@pytest.mark.parametrize("name", list(CASES))
def test_sampler_on_every_fit_of_a_case(H, O, name):
    """The restated sampler (hiprec_weight.py section 1) over every fit of the case: the 100 points lie in the closed cell and
    their mapped coordinates in [-1, 1]; no two fits of the case share a key -- a cell's P fit and its children, child 0 that
    shares its parent's bmin, the same cell at another degree; the key is ora_weight_key's and the points are the oracle's bit for
    bit (which pins the restatement of the definition, nothing more)."""
    L = _ora_weight_api(O)
    arrays = guided(H, O, name)[4]
    fitsets = {}
    for lo, hi, depth, degree, _ in arrays:
        fitsets.setdefault((depth, degree), {})[lo.tobytes() + hi.tobytes()] = (lo, hi)
    keys, n_fits = set(), 0
    pt64 = np.zeros(3)
    for (depth, degree), cells in fitsets.items():
        lo = np.array([c[0] for c in cells.values()], np.float32)
        hi = np.array([c[1] for c in cells.values()], np.float32)
        pt, x = W.sample_points(lo, hi, depth, degree)
        assert pt.shape == (len(lo), 100, 3)
        assert (pt >= lo[:, None, :]).all() and (pt <= hi[:, None, :]).all()
        assert (np.abs(x) <= 1).all()
        # the closed cell maps onto [-1, 1], not onto half of it: 300 coordinates uniform in [-1, 1] all within 0.5 has probability 2^-300
        assert (np.abs(x).max(axis=(1, 2)) > 0.5).all()
        k = W.weight_key(lo, depth, degree)
        keys |= set(int(v) for v in k)
        n_fits += len(lo)
        for j in range(0, len(lo), max(1, len(lo) // 8)):            # a spread of the cells through the oracle, all 100 points
            assert int(k[j]) == L.ora_weight_key(_f3(lo[j]), depth, degree)
            for i in range(100):
                L.ora_weight_point(_f3(lo[j]), _f3(hi[j]), depth, degree, i, pt64.ctypes.data_as(C.POINTER(C.c_double)))
                assert pt64.tobytes() == pt[j, i].astype(np.float64).tobytes(), (name, depth, degree, j, i)
    assert len(keys) == n_fits, "two fits of the case share a sampler key"
    p_child0 = [(lo, depth, degree) for lo, hi, depth, degree, _ in arrays[-9:-8]]
    for lo, depth, degree in p_child0:                                # the last job's P fit against its child 0 and the next depth
        assert W.weight_key(lo, depth, degree)[0] != W.weight_key(lo, depth + 1, degree - 1)[0]
        assert W.weight_key(lo, depth, degree)[0] != W.weight_key(lo, depth + 1, degree)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_mean_and_weight_piecewise(H, O, name):
    """ora_weight_mean of every fit array of the case (the float64 arrays the oracle's jobs produced) within the mean's bound of the
    long-double mean of the long-double array the fit history gives; ora_weight_from_mean of that float64 mean within the
    weight's bound (the libm call and the three roundings in front of it) of the long-double weight -- exactly 0 where
    m > sqrt 3 under the integer strength, exactly 1 in the NaN branch of the fractional one."""
    L = _ora_weight_api(O)
    wt = weighting_of(name)
    fits = fits_of(name)
    blk, st, seen, rounds, arrays = guided(H, O, name)
    # the arrays in job order with their provenance: the replay's history at the time is in the items the replay itself formed
    rep = B.Guided(*case_spec(name)[:4], fits=fits, weighting=wt)
    worst_m = worst_w = 0.0
    tags = {"zero": 0, "nan": 0, "excluded": 0}
    it = iter(arrays)
    for jobs, headers in rounds:
        coarse = rep.s.counts["rounds"] == 0
        items = []
        for n, lo, hi, err, degree, depth, jc in jobs:
            p0 = 2 if coarse else rep.s.hist[n][0]
            items.append((lo, hi, depth, 2, 2, "C") if coarse else (lo, hi, depth, p0, degree + 1, "P"))
            if not coarse:
                items += [B.corner_aabb(lo, hi, i) + (depth + 1, degree, degree, "H") for i in range(8)]
        means = wt.means(fits, items)
        for item, (mean, mb) in zip(items, means):
            lo, hi, depth, degree, co = next(it)
            assert np.array_equal(lo, item[0]) and (depth, degree) == (item[2], item[4])
            m64 = L.ora_weight_mean(co.ctypes.data_as(C.POINTER(C.c_double)), degree, _f3(lo), _f3(hi), depth)
            ratio = float(abs(R.LD(m64) - abs(mean))) / mb
            worst_m = max(worst_m, ratio)
            assert ratio <= 1, (name, depth, degree, m64, float(mean), mb)
            w64 = L.ora_weight_from_mean(wt.wtype, wt.strength, m64)
            w, wb, tag = W.weight_from_mean(wt.wtype, wt.strength, R.LD(m64), 0.0)
            if tag:
                tags[tag] += 1
            if tag == "zero":
                assert w64 == 0.0 and m64 > np.sqrt(3.0)
            elif tag == "nan":
                assert w64 == 1.0 and m64 > np.sqrt(3.0)
            elif tag != "excluded":
                ratio = float(abs(R.LD(w64) - w)) / wb
                worst_w = max(worst_w, ratio)
                assert ratio <= 1, (name, m64, w64, float(w), wb)
        rep.check_round(jobs, headers)
    print("\n%s: %d arrays, oracle mean %.3g of its bound, oracle weight %.3g of its bound, weight 0 %d, NaN branch %d, excluded %d"
          % (name, len(arrays), worst_m, worst_w, tags["zero"], tags["nan"], tags["excluded"]))
    SEEN[name + "/piecewise"] = tags


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_weighted_create_equals_the_free_replay(O, name):
    """Tree.create of the oracle with nearness weighting, one shot, against replay_free grown from the weighted long-double errors:
    the assertions of test_oracle_create_equals_the_free_replay -- every node, the counts, zero undecided decisions and selections,
    the stop consistent with the true (weighted) total, every leaf's rows against the fits that formed them."""
    spec, root, target, K, _ = case_spec(name)
    blk, st = oracle_create(O, name)
    rep = free_replay(name, st["rounds"])
    wseen = rep["weighting"].seen
    print("\n%s: rounds %d, jobs past round 0 %d, P %d, H %d, max degree %d, max depth %d, min margin %.3g bounds, weighted arrays %d "
          "(weight 0: %d, NaN branch: %d, excluded: %d)"
          % (name, st["rounds"], st["jobs"] - 4096, st["p_refines"] - 4096, st["h_refines"], rep["degree"][rep["degree"] < 13].max(),
             rep["depth"].max(), rep["min_margin"], wseen["arrays"], wseen["zero"], wseen["nan"], wseen["excluded"]))
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0, (rep["undecided_decisions"], rep["undecided_selections"])
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"], (float(rep["true_total"]), rep["true_bound"], rep["B"], target)
    rows = B.check_leaf_rows(blk, spec, rep["history"], fits=fits_of(name))
    print("%s: leaf rows %.3g of the bound, longest chain of P-appends %d" % (name, rows["worst"], rows["chain"]))
    assert rows["worst"] <= 1
    SEEN[name] = dict(h_depth=int(rep["depth"][rep["degree"] == 13].max()), jobs=st["jobs"])


@pytest.mark.parametrize("name", list(CASES))
def test_host_scheduler_under_check_round_weighted(H, O, name):
    """The product's host scheduler with the oracle's weighted job numerics, every round under check_round: all nine weighted errors
    of a job within their bounds, a coarse job's eight other slots +0.0, the selection, the decisions, then the block's tree, the
    statistics, total_error bit for bit from the restated statements and within B of the true total, every leaf's rows -- and the
    block is the oracle's one-shot block."""
    spec, root, target, K, _ = case_spec(name)
    blk, st, seen, _, _ = guided(H, O, name)
    print("\n%s: rounds %d, job errors %.3g of the bound, smallest decision margin %.3g bounds, undecided %d, ties at the K-th place %d, "
          "rounds below K entries %d, total drift %.3g of B (B %.3g)" % (name, st["rounds"], seen["job_error"], seen["min_margin"],
                                                                        seen["undecided"], seen["selection_ties"], seen["small_rounds"],
                                                                        seen["drift_over_B"], seen["B"]))
    rows = B.check_leaf_rows(blk, spec, seen["history"], fits=fits_of(name))
    assert rows["worst"] <= 1 and seen["job_error"] <= 1
    assert seen["undecided"] == 0 and seen["selection_ties"] == 0
    assert blk == oracle_create(O, name)[0]
    SEEN[name + "/guided"] = seen


def test_weighted_cases_reach_what_they_are_for(H, O):
    """Between them: both weighting types; strength 3 and a fractional one; a weighted P fit on an array that already carries two
    appends; a weighted H below depth 5; an array of degree >= 6 through the mean; cells with m > sqrt 3 that take weight 0
    exactly under the integer strength and the NaN branch under the fractional one; a round with fewer than K queued entries; and
    at most 2 % of a case's jobs excluded as undecided by construction."""
    for name in CASES:
        if name not in SEEN:
            test_oracle_weighted_create_equals_the_free_replay(O, name)
        if name + "/guided" not in SEEN:
            test_host_scheduler_under_check_round_weighted(H, O, name)
    ws = [c[5] for c in CASES.values()]
    assert {w[0] for w in ws} == {W.POLYNOMIAL, W.EXPONENTIAL}
    assert any(w[1] == 3.0 for w in ws) and any(not float(w[1]).is_integer() for w in ws)
    seen = {n: weighting_of(n).seen for n in CASES}
    assert max(s["appends_carried"] for s in seen.values()) >= 2
    assert max(s["max_degree"] for s in seen.values()) >= 6
    assert max(SEEN[n]["h_depth"] for n in CASES) >= 5
    zero = [n for n in CASES if CASES[n][5] == (W.POLYNOMIAL, 3.0) and seen[n]["zero"] > 0]
    nan = [n for n in CASES if not float(CASES[n][5][1]).is_integer() and seen[n]["nan"] > 0]
    assert zero and nan, (zero, nan)
    assert sum(SEEN[n + "/guided"]["small_rounds"] for n in CASES) > 0
    for n in CASES:
        assert seen[n]["excluded"] <= 0.02 * SEEN[n]["jobs"], (n, seen[n]["excluded"])


# ---------------------------------------------------------------------------------------------------------------- mutants
MUTANT_CASES = {"w_new_rows": "aniso-exp3", "w_child_parent": "aniso-exp3", "w_coarse_nine": "cube-poly3", "w_d3": "cube-poly3",
                "w_noabs": "cube-poly3", "w_noclamp": "cube-poly3", "w_exp_plus": "aniso-exp3", "w_99": "aniso-exp3",
                "w_shift1": "aniso-exp3", "w_key_nodegree": "aniso-exp3"}
# Mutants whose errors stay on the same side of every decision and selection of these cases, which are far from ties by
# construction: a coarse job is forced to P whatever its other eight slots hold; without the clamp the far cells' errors are negative
# instead of 0 and stay at the end of the order; one sample in a hundred moves the weights by a percent.  Only check_round sees them.
TREE_BLIND = ("w_coarse_nine", "w_noclamp", "w_99")


@pytest.mark.parametrize("mutant", list(B.WEIGHT_MUTANTS))
def test_mutants_of_the_weighting_are_caught(H, O, mutant):
    """Each mutant of the weighting -- the mean over the appended rows only, a child weighted with its parent's array, all nine
    headers of a coarse job weighted, d = 3 for sqrt 3, no abs, the clamp dropped, exp with + s, 99 samples, 1 << depth in the
    mapping, the key without the degree -- fails check_round on the host scheduler's rounds of its case, by more than the bounds;
    the unmutated replay passed the same rounds (guided() ran them).  All but TREE_BLIND grow another tree than the oracle's in
    the free replay too.  A check loose enough to admit one of them would fail here."""
    name = MUTANT_CASES[mutant]
    spec, root, target, K, weighting = case_spec(name)
    if mutant not in TREE_BLIND:
        blk, st = oracle_create(O, name)
        rep = B.replay_free(spec, root, target, K, st["rounds"], fits=fits_of(name), weighting=weighting, mutant=mutant)
        with pytest.raises(AssertionError):
            B.same_tree(blk, rep)
    rounds = guided(H, O, name)[3]
    g = B.Guided(spec, root, target, K, mutant=mutant, fits=fits_of(name), weighting=weighting)
    with pytest.raises(AssertionError) as caught:
        for jobs, headers in rounds:
            g.check_round(jobs, headers)
    print("\n%s on %s: %s" % (mutant, name, str(caught.value).split("\n")[0][:160]))
    assert g.s.weighting.mutant == mutant
