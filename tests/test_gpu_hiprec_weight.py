"""Nearness-weighted Create on the device against the extended-precision replay (tests/hiprec_build.py with tests/hiprec_weight.py):
the stepwise Build with the GPU's fits, fit_weight_kernel's means and the host's weights under check_round every round, and
one-shot create_block -- device frontier (fr_weigh_kernel), host scheduler, 2 and 4 simulated ranks (the row exchange), the
grid-selection replica mode, the other reduction order -- against replay_free.  One replay per case, shared by every variant: the
long-double work runs on the CPU and is the cost, the GPU side of each test is milliseconds to a few seconds.  The byte-identity
tests pin weighted builds to the oracle; these pin them -- and through the CPU module the oracle -- to Octree.cpp and the
sampler's definition."""
import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
import hiprec_weight as W
from test_hiprec_weight_cpu import CASES, case_spec, configs, fits_of, weighting_of

pytestmark = pytest.mark.gpu

# The largest observed figure / bound of the module, printed at its end.
WORST = {"leaf rows": 0.0, "job errors": 0.0, "decision margin": np.inf, "total drift / B": 0.0}
_RUNS = {}
VARIANTS = ("device", "host", "ranks2", "ranks4", "grid2")


def _stepwise(H, ctx, name, left=False):
    """Build.select / jobs / compute / results_host / apply on the GPU under check_round -> (block, stats, Guided.finish's
    observations, fits, weighting).  results_host returns the weighted headers: all nine of a job are checked here."""
    spec, root, target, K, weighting = case_spec(name)
    fits = B.Fits(spec, root, left=True) if left else fits_of(name)
    wt = W.Weighting(*weighting) if left else weighting_of(name)
    b, f = H.Build(configs(H, None, name)[0], K, 0, 1), H.Field.analytic(spec)
    g = B.Guided(spec, root, target, K, left=left, fits=fits, weighting=wt)
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
    WORST["job errors"] = max(WORST["job errors"], seen["job_error"])
    WORST["decision margin"] = min(WORST["decision margin"], seen["min_margin"])
    WORST["total drift / B"] = max(WORST["total drift / B"], seen["drift_over_B"])
    return blk, st, seen, fits, wt


@pytest.fixture(scope="module")
def runs(H, ctx):
    """name -> the stepwise run on the default context, made on first use."""
    def get(name, left=False):
        if (name, left) not in _RUNS:
            _RUNS[name, left] = _stepwise(H, ctx, name, left)
        return _RUNS[name, left]
    yield get
    print("\nweighted build replay, largest figure / bound: leaf rows %.3g, job errors %.3g, smallest decision margin %.3g bounds, "
          "total drift / B %.3g" % (WORST["leaf rows"], WORST["job errors"], WORST["decision margin"], WORST["total drift / B"]))


def _rows(blk, name, history, fits):
    got = B.check_leaf_rows(blk, case_spec(name)[0], history, fits=fits)
    WORST["leaf rows"] = max(WORST["leaf rows"], got["worst"])
    assert got["worst"] <= 1, (name, got["worst"])
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_stepwise_weighted_build_under_check_round(H, ctx, runs, name):
    """The stepwise Build of a weighted config with the GPU's numerics, every round under check_round: all nine weighted errors of
    every job within their bounds (the fit's, fit_weight_kernel's mean of its own array, the host's pow / exp), a coarse job's
    eight other slots +0.0, the selection, every decision the one float64 takes; then the block's tree, the statistics,
    total_error bit for bit from the restated float64 statements and within B of the true weighted total, and every leaf's rows
    against the fits that formed them."""
    blk, st, seen, fits, wt = runs(name)
    _rows(blk, name, seen["history"], fits)
    assert seen["job_error"] <= 1
    assert seen["selection_ties"] == 0 and seen["undecided"] == 0
    assert wt.seen["excluded"] == 0


def _one_shot(H, ctx, monkeypatch, name, variant):
    spec, root, target, K, _ = case_spec(name)
    cfg = configs(H, None, name)[0]
    if K > 4096 and variant != "host":
        # The device frontier carries rounds of up to 4096 jobs; a larger K goes to the host scheduler.  The case never queues more
        # than 4096 entries, so K = 4096 selects what K = 8192 selects: the same replay serves both.
        K = 4096
    if variant == "grid2":
        # the selection as a grid, as test_gpu_configs.test_weighted_build_sharded_with_the_grid_selection forces it
        monkeypatch.setenv("HPSDF_FRONTIER_INLINE_NODES", "0")
    if variant in ("ranks2", "ranks4", "grid2"):
        from test_gpu_configs import _create_on_simulated_ranks
        out = _create_on_simulated_ranks(H, int(variant[-1]), cfg, lambda c: H.Field.analytic(spec), K)
        assert all(blk == out[0][0] for blk, _ in out), "the ranks' blocks differ"
        assert all(st["device_frontier"] == 1 for _, st in out)
        if variant == "grid2":
            assert H.create_block(ctx, cfg, H.Field.analytic(spec), K)[0] == out[0][0]
        return out[0]
    monkeypatch.setenv("HPSDF_HOST_FRONTIER", "1" if variant == "host" else "0")
    return H.create_block(ctx, cfg, H.Field.analytic(spec), K)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_one_shot_weighted_create_against_the_free_replay(H, ctx, runs, monkeypatch, name, variant):
    """create_block of a weighted config, one shot, against replay_free grown from the weighted long-double errors for the build's
    own number of rounds: the tree node by node, rounds / jobs / P / H / dropped, every leaf's rows -- a stale copied row on a
    rank shows here --, the stop consistent with the true total, total_error bit for bit the float64 statements restated from the
    errors the stepwise run checked; every rank's block identical."""
    spec, root, target, K, _ = case_spec(name)
    _, sst, seen, fits, wt = runs(name)
    blk, st = _one_shot(H, ctx, monkeypatch, name, variant)
    rep = _RUNS.get(("free", name))
    if rep is None:
        rep = _RUNS["free", name] = B.replay_free(spec, root, target, K, st["rounds"], fits=fits, weighting=wt)
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"]
    assert st["device_frontier"] == (0 if variant == "host" else 1)
    _rows(blk, name, rep["history"], fits)
    assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes(), (st["total_error"], seen["f64_total"])


def test_one_shot_weighted_create_in_the_other_reduction_order(H, ctx, runs):
    """hpsdf_set_reduction_order(1) through a whole weighted build, against a replay whose fields are evaluated in that order."""
    name = "aniso-exp3"
    spec, root, target, K, _ = case_spec(name)
    H.set_reduction_order(1)
    try:
        _, _, seen, fits, wt = runs(name, left=True)
        blk, st = H.create_block(ctx, configs(H, None, name)[0], H.Field.analytic(spec), K)
    finally:
        H.set_reduction_order(0)
    rep = B.replay_free(spec, root, target, K, st["rounds"], left=True, fits=fits, weighting=wt)
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0 and rep["stop_consistent"]
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    _rows(blk, name, rep["history"], fits)
    assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes()
