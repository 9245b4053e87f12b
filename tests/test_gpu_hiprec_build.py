"""Create on the device against the extended-precision replay of the build (tests/hiprec_build.py): the stepwise Build with the
GPU's fits under check_round every round, and one-shot create_block -- device frontier, host scheduler, every fit mode, 2 and 8
simulated ranks, the other reduction order -- against replay_free.  One replay per case, shared by every variant: the long-double
work runs on the CPU and is the cost, the GPU side of each test is milliseconds.  The byte-identity tests pin Create to the
oracle; these pin it -- and through the CPU module the oracle -- to Octree.cpp's schedule and to the mathematics."""
import numpy as np
import pytest

import hiprec as R
import hiprec_build as B
from test_hiprec_build_cpu import CASES, FREE_CASES, TIE_CASES, case_spec, fits_of

pytestmark = pytest.mark.gpu

# The largest observed figure / bound of the module, printed at its end.
WORST = {"leaf rows": 0.0, "job errors": 0.0, "decision margin": np.inf, "total drift / B": 0.0}
_RUNS = {}
VARIANTS = ("device", "host", "exact", "split2", "fast", "ranks2", "ranks8")


def _stepwise(H, ctx, name, left=False):
    """Build.select / jobs / compute / results_host / apply on the GPU under check_round -> (block, stats, Guided.finish's
    observations, fits).  The nine errors that reach the decision are checked here, the alternative's included."""
    spec, root, target, K = case_spec(name)
    fits = B.Fits(spec, root, left=True) if left else fits_of(name)
    b, f = H.Build(H.make_config(target, *root), K, 0, 1), H.Field.analytic(spec)
    g = B.Guided(spec, root, target, K, left=left, fits=fits)
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
    return blk, st, seen, fits


@pytest.fixture(scope="module")
def runs(H, ctx):
    """name -> the stepwise run on the default context, made on first use."""
    def get(name, left=False):
        if (name, left) not in _RUNS:
            _RUNS[name, left] = _stepwise(H, ctx, name, left)
        return _RUNS[name, left]
    yield get
    print("\nbuild replay, largest figure / bound: leaf rows %.3g, job errors %.3g, smallest decision margin %.3g bounds, total drift / B %.3g"
          % (WORST["leaf rows"], WORST["job errors"], WORST["decision margin"], WORST["total drift / B"]))


@pytest.fixture(scope="module")
def contexts(H, ctx):
    exact = H.Context(0)
    exact.set_fit_mode(H.FIT_EXACT)
    split = H.Context(0)
    split.set_fit_mode(H.FIT_SPLIT)
    split.set_split_min_degree(2)
    fast = H.Context(0)
    fast.set_fast_fit(True)
    yield {"device": ctx, "host": ctx, "exact": exact, "split2": split, "fast": fast}
    for c in (exact, split, fast):
        c.close()


def _rows(blk, name, history, fits):
    spec = case_spec(name)[0]
    got = B.check_leaf_rows(blk, spec, history, fits=fits)
    WORST["leaf rows"] = max(WORST["leaf rows"], got["worst"])
    assert got["worst"] <= 1, (name, got["worst"])
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_stepwise_build_under_check_round(H, ctx, runs, name):
    """The stepwise Build with the GPU's fits, every round under check_round: the selection within the bounds of the K-th error
    (the tie cases have reference errors closer than their bounds there), the jobs in node order with the replay's boxes, degrees
    and queued errors, all nine errors of every job within their bounds, every decided decision the one float64 takes; then the
    block's tree, the statistics, total_error bit for bit from the restated float64 statements and within B of the true total, and
    every leaf's rows against the fits that formed them."""
    blk, st, seen, fits = runs(name)
    _rows(blk, name, seen["history"], fits)
    assert seen["job_error"] <= 1
    if name in TIE_CASES:
        assert seen["selection_ties"] > 0
    else:
        assert seen["selection_ties"] == 0 and seen["undecided"] == 0


def test_stepwise_build_with_the_matrix_core_fits(H, contexts):
    """FIT_FAST through the stepwise API (every fit of degree >= 4 on the matrix cores; the case reaches degree 6): its errors are
    not the exact kernel's bits but lie within the same bounds, so every check of check_round holds as it stands -- total_error is
    then the restated total of ITS errors."""
    blk, st, seen, fits = _stepwise(H, contexts["fast"], "aniso-sphere9")
    _rows(blk, "aniso-sphere9", seen["history"], fits)
    assert st["fit_mode"] == H.FIT_FAST


def _one_shot(H, contexts, monkeypatch, name, variant):
    spec, root, target, K = case_spec(name)
    cfg = H.make_config(target, *root)
    if K > 4096 and variant != "host":
        # The device frontier carries rounds of up to 4096 jobs (kFrJobs, csrc/frontier_dev.hpp); a larger K goes to the host scheduler.
        # cube-allK never queues more than 4096 entries, so K = 4096 selects what K = 8192 selects: the same replay serves both.
        K = 4096
    if variant.startswith("ranks"):
        from test_gpu_configs import _create_on_simulated_ranks
        out = _create_on_simulated_ranks(H, int(variant[5:]), cfg, lambda c: H.Field.analytic(spec), K)
        assert all(blk == out[0][0] for blk, _ in out)
        return out[0]
    monkeypatch.setenv("HPSDF_HOST_FRONTIER", "1" if variant == "host" else "0")
    return H.create_block(contexts[variant], cfg, H.Field.analytic(spec), K)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(FREE_CASES))
def test_one_shot_create_against_the_free_replay(H, contexts, runs, monkeypatch, name, variant):
    """create_block, one shot, against replay_free grown from long-double errors alone for the build's own number of rounds: the
    tree node by node, rounds / jobs / P / H / dropped, every leaf's rows (the lower rows of a split or matrix-core fit are other
    bits within the same bound), the stop consistent with the true total, and total_error bit for bit the float64 statements
    restated from the errors the stepwise run checked.  FIT_FAST's errors are other bits within the same bounds: its tree must be
    the replay's because no decision or selection of these cases is undecided, and its total lies within B of the true one."""
    spec, root, target, K = case_spec(name)
    _, sst, seen, fits = runs(name)
    blk, st = _one_shot(H, contexts, monkeypatch, name, variant)
    rep = _RUNS.get(("free", name))
    if rep is None:
        rep = _RUNS["free", name] = B.replay_free(spec, root, target, K, st["rounds"], fits=fits)
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    assert rep["stop_consistent"]
    assert st["device_frontier"] == (0 if variant == "host" else 1)
    _rows(blk, name, rep["history"], fits)
    if variant == "fast":
        drift = float(abs(R.LD(st["total_error"]) - rep["true_total"]))
        assert drift <= rep["B"] + rep["true_bound"], (drift, rep["B"])
    else:
        assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes(), (st["total_error"], seen["f64_total"])


def test_one_shot_create_in_the_other_reduction_order(H, O, ctx, runs):
    """hpsdf_set_reduction_order(1): the leftAssoc instantiations through the whole build, against a replay whose fields are
    evaluated in that order."""
    name = "aniso-sphere"
    spec, root, target, K = case_spec(name)
    H.set_reduction_order(1)
    try:
        _, _, seen, fits = runs(name, left=True)
        blk, st = H.create_block(ctx, H.make_config(target, *root), H.Field.analytic(spec), K)
    finally:
        H.set_reduction_order(0)
    rep = B.replay_free(spec, root, target, K, st["rounds"], left=True, fits=fits)
    assert rep["undecided_decisions"] == 0 and rep["undecided_selections"] == 0 and rep["stop_consistent"]
    B.same_tree(blk, rep)
    for k in ("rounds", "jobs", "p_refines", "h_refines", "dropped"):
        assert st[k] == rep["counts"][k], k
    _rows(blk, name, rep["history"], fits)
    assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes()


def test_stop_rule_drift_on_the_device(H, ctx, runs):
    """The device's running total (fr_round_kernel's chain workgroup) reproduces the reference's float64 drift: target 1e-10, the
    total ends below it -- negative -- while the true sum of the leaves' errors is a hundred times the target."""
    name = "unit-sphere9"
    spec, root, target, K = case_spec(name)
    _, _, seen, _ = runs(name)
    _, st = H.create_block(ctx, H.make_config(target, *root), H.Field.analytic(spec), K)
    assert st["device_frontier"] == 1
    assert np.float64(st["total_error"]).tobytes() == np.float64(seen["f64_total"]).tobytes()
    assert st["total_error"] < target < float(seen["true_total"]) - seen["true_bound"]
    assert seen["drift"] <= seen["B"]
