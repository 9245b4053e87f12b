"""The context-stream contract of the device entry points (include/hpsdf.h, "The stream contract"): every entry launches on the
context's stream, in the order of the calls, and the entries the header calls asynchronous return without a host wait.

Every other GPU test hands over complete inputs and reads outputs after a full synchronisation, which hides WHEN the work runs.  Here a
context lives on a caller's stream S (or S is the library's own stream), and everything -- a calibrated delay, a device-to-device copy of
the real inputs P1 over a valid decoy P0, the entry, a clone of the outputs, a copy of a third valid set P2 over the inputs -- is queued on
S with no host wait; only then is S synchronised and the clone compared, byte for byte, with what the same entry returns for P1 when
called the ordinary synchronised way on a second, untouched context.  tests/stream_order.py holds the machinery; a mismatch says whether
P0's answer (read too early), P2's (read too late) or the outputs' 7.0 fill (written too late) came back."""
import os
import re
import threading

import numpy as np
import pytest
import torch

import simplify_reference as SR
import stream_order as SO
from conftest import ROOT
from helpers import synthetic_block
from stream_order import ENTRIES, Step, run_pattern, synchronised, three_sets
from test_integrate_cpu import synthetic_iso
from test_integrate_pair_cpu import general_pose

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "csrc")
# Query's launch paths (csrc/launch.hpp, launchQuery in csrc/kernels.hip; test_the_sizes_reach_the_launch_paths reads them there):
FEW_POINTS = 256                  # kQueryFewPoints: up to here one launch of the few-point kernel
BIG_TILE, BIG_WGS = 1024, 256     # trees with a depth-4 top table: tiles of 1024 points over at most 256 workgroups
N_FEW, N_TILES, N_MANY = 200, 3000, 300_000   # the few-point kernel; a few tiles; more than one tile per workgroup on the 1024-wide path
DEGREES = {3: [3, 2, 1, 0, 3, 3, 2, 1], 5: [5, 4, 3, 2, 1, 0, 5, 4], 12: [12, 7, 3, 2, 9, 0, 5, 6]}


def test_the_sizes_reach_the_launch_paths():
    with open(os.path.join(CSRC, "launch.hpp")) as f:
        assert int(re.search(r"kQueryFewPoints = (\d+);", f.read()).group(1)) == FEW_POINTS
    with open(os.path.join(CSRC, "kernels.hip")) as f:
        src = f.read()
    assert "const unsigned tile = big ? %du : 256u;" % BIG_TILE in src
    assert re.search(r'getenv\("HPSDF_QUERY_GENERAL_WGS"\); return e \? .*? : (\d+)u; \}', src).group(1) == str(BIG_WGS)
    assert N_FEW <= FEW_POINTS < N_TILES                                   # one few-point launch; the tiled kernels
    assert 2 * 256 < N_TILES and 2 * BIG_TILE < N_TILES                     # a few tiles on either path, the last one ragged
    assert N_MANY > BIG_TILE * BIG_WGS and N_MANY % BIG_TILE != 0           # a second tile for some workgroups, the last one ragged


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def delay():
    d = SO.Delay()
    print("delay: %s x %d = %.1f ms" % (d.kind, d.count, d.ms))
    return d


@pytest.fixture(scope="module")
def ref_ctx(H):
    """the second, untouched context: every expected value is a synchronised call on it"""
    c = H.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def blocks(H, ref_ctx):
    out = {"inline": H.create_block(ref_ctx, H.make_config(1e-5), H.Field.union3(), 1024)[0],     # golden C2_union3_1e-5
           "deg4": H.create_block(ref_ctx, H.make_config(1e-7), H.Field.union3(), 1024)[0],       # golden A1_union3_1e-7_K1024
           "deg12": synthetic_block(np.random.default_rng(1201), DEGREES[12], 1),
           "deg12b": synthetic_block(np.random.default_rng(1213), DEGREES[12], 1),
           "A": synthetic_block(np.random.default_rng(1217), DEGREES[5], 2),
           "B": synthetic_block(np.random.default_rng(1223), DEGREES[3], 2)}
    info = {k: H.DeviceTree(ref_ctx, v).info() for k, v in out.items()}
    assert info["inline"]["max_degree"] == 2 and info["inline"]["max_depth"] == 4     # every leaf in the depth-4 top table
    assert info["deg4"]["max_degree"] == 4 and info["deg12"]["max_degree"] == 12 == info["deg12b"]["max_degree"]
    return out


@pytest.fixture(scope="module")
def refs(H, ref_ctx, blocks):
    """(entry, tree, n, seed) -> (the three input sets, the synchronised outputs for each), computed once"""
    cache, trees = {}, {}

    def get(entry, tree, n, seed=0, two_pass=False):
        key = (entry, tree, n, seed, two_pass)
        if key not in cache:
            if tree not in trees:
                trees[tree] = H.Field.union3() if tree == "union3" else H.DeviceTree(ref_ctx, blocks[tree])
            sets = three_sets(ENTRIES[entry].make, n, 9000 + 10 * seed)
            with two_pass_env(two_pass):
                cache[key] = (sets, synchronised(H, ref_ctx, ENTRIES[entry], trees[tree], sets, n))
        return cache[key]

    return get


class two_pass_env:
    """HPSDF_QUERY_TWO_PASS=1 (read at every launch): the scan + second-pass route on a tree that would take the one-launch path"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["HPSDF_QUERY_TWO_PASS"] = "1"

    def __exit__(self, *a):
        if self.on:
            del os.environ["HPSDF_QUERY_TWO_PASS"]


class on_stream:
    """A context on a caller's stream ("caller"), or a context with its own stream reached through hpsdf_ctx_stream ("owned")."""

    def __init__(self, H, kind="caller"):
        if kind == "caller":
            self.S = torch.cuda.Stream()
            self.ctx = H.Context(0, self.S.cuda_stream)
        else:
            self.ctx = H.Context(0)
            self.S = torch.cuda.ExternalStream(H.lib().hpsdf_ctx_stream(self.ctx.handle))

    def __enter__(self):
        return self.ctx, self.S

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.ctx.close()


NO_WAIT = "the entry waited for the stream on the host: the delay queued ahead of it had ended when it returned"


# ------------------------------------------------------------------------------------------------------------ Query
@pytest.mark.parametrize("entry", ["query", "query_with_gradient"])
@pytest.mark.parametrize("n", [N_FEW, N_TILES, N_MANY])
@pytest.mark.parametrize("tree", ["inline", "deg4", "deg4-two-pass", "deg12"])
def test_query_on_a_caller_stream(H, blocks, refs, delay, tree, n, entry):
    """hpsdf_query_device and hpsdf_query_gradient_device on a caller's stream: the all-inline kernels, the one-launch path that finishes
    degrees 4-5 in the workgroup (and the scan + second pass on the same tree), the scan + second pass of a degree-12 tree; the few-point
    kernel, a few tiles, more than one tile a workgroup.  Catches: a launch on stream 0 or on a stream of the library's (P0's answer or
    the fill); a second pass or scan queued elsewhere than the first (a mixture); a host wait (the delay has ended on return)."""
    name, two_pass = tree.replace("-two-pass", ""), tree.endswith("two-pass")
    sets, want = refs(entry, name, n, two_pass=two_pass)
    with on_stream(H) as (ctx, S), two_pass_env(two_pass):
        step, pending = run_pattern(H, ctx, S, delay, ENTRIES[entry], H.DeviceTree(ctx, blocks[name]), sets, n)
    step.check(want, (entry, tree, n))
    assert pending, NO_WAIT


@pytest.mark.parametrize("n", [N_FEW, N_TILES, N_MANY])
def test_query_on_the_library_owned_stream(H, blocks, refs, delay, n):
    """The same with the caller's work queued on the context's OWN stream (hpsdf_ctx_stream): that stream is non-blocking, so the null
    stream does not wait for it.  Catches a launch on stream 0 (P0's answer) and a host wait."""
    sets, want = refs("query", "deg12", n)
    with on_stream(H, "owned") as (ctx, S):
        step, pending = run_pattern(H, ctx, S, delay, ENTRIES["query"], H.DeviceTree(ctx, blocks["deg12"]), sets, n)
    step.check(want, ("query, owned stream", n))
    assert pending, NO_WAIT


# ------------------------------------------------------------------------------------------------------------ the other point and ray entries
@pytest.mark.parametrize("entry", ["query_gradient", "query_hessian", "project", "cast_rays", "field_eval"])
def test_point_and_ray_entries(H, blocks, refs, delay, entry):
    """3 000 items on the degree-4 tree (the field: union3 itself).  Catches a launch on stream 0 or another stream (P0's answer, the
    fill) and a host wait."""
    name = "union3" if entry == "field_eval" else "deg4"
    sets, want = refs(entry, name, N_TILES)
    if entry == "cast_rays":
        assert (want[1][0] == H.CAST_HIT).mean() > 0.9, np.bincount(want[1][0])
    with on_stream(H) as (ctx, S):
        obj = H.Field.union3() if entry == "field_eval" else H.DeviceTree(ctx, blocks[name])
        step, pending = run_pattern(H, ctx, S, delay, ENTRIES[entry], obj, sets, N_TILES)
    step.check(want, (entry, N_TILES))
    assert pending, NO_WAIT


@pytest.mark.parametrize("entry", ["query_bounds", "query_bounds_grid"])
def test_the_first_bounds_call_on_a_tree_and_the_next(H, blocks, refs, delay, entry):
    """The FIRST bounds call on a freshly uploaded tree is made behind the delay: it builds the tree's cached constants on the context
    stream and waits for them (the header says so: no no-wait assertion), then launches.  The second call only launches: no host wait.
    Catches: the constants built or the bounds launched on stream 0 or another stream (the fill, P0's answer; constants read before they
    are built give a mixture), the wait for the constants removed while the depth array they are built from is freed."""
    sets, want = refs(entry, "deg4", N_TILES)
    assert set(np.unique(want[1][2])) == {H.BOUNDS_OK}
    with on_stream(H) as (ctx, S):
        tree = H.DeviceTree(ctx, blocks["deg4"])
        first, _ = run_pattern(H, ctx, S, delay, ENTRIES[entry], tree, sets, N_TILES)
        second, pending = run_pattern(H, ctx, S, delay, ENTRIES[entry], tree, sets, N_TILES)
    first.check(want, (entry, "first call"))
    second.check(want, (entry, "second call"))
    assert pending, NO_WAIT


# ------------------------------------------------------------------------------------------------------------ entries that return host results
def _host_entries(H, blocks):
    A, B = blocks["A"], blocks["B"]
    iso_a, iso_b = synthetic_iso(H, A), synthetic_iso(H, B)
    pose = general_pose(H, (0.1, 0.05, 0.12))
    poses = np.stack([general_pose(H, t) for t in ((0.1, 0.05, 0.12), (0.31, 0.17, -0.12), (0.0, 0.0, 0.0), (-0.2, 0.1, 0.3), (0.05, -0.1, 0.08))])
    merge = SR.exact_merge_block(np.random.default_rng(41), [4, 4, 4, 1, 2, 4, 2, 1], 4)[0]
    return {
        "integrate": lambda ctx, tA, tB: tA.integrate(iso_a, 4, 2, 1 << 13, cells=True),
        "integrate_pair": lambda ctx, tA, tB: tA.integrate_pair(tB, H.PAIR_INTERSECTION, pose, iso_a, iso_b, 4, 2, 1 << 13, 256, cells=True),
        "clearance": lambda ctx, tA, tB: tA.clearance(tB, pose, iso_a, 4, 0.0, 1 << 13, 256, cells=True),
        "clearance_batch": lambda ctx, tA, tB: tA.clearance_batch(tB, poses, iso_a, 3, 0.0, 1 << 13, 256),
        "simplify": lambda ctx, tA, tB: (H.simplify(ctx, merge, 1e-9), H.simplify(ctx, blocks["deg4"], 1e-3)),
    }


def _same_host_result(got, want, what):
    if isinstance(got, tuple):                                                   # simplify: ((block, stats), (block, stats))
        assert got == want, (what, [g[1] for g in got], [w[1] for w in want])
        return
    assert got.raw == want.raw, (what, "struct", got, want)
    if getattr(got, "cells", None) is not None:
        assert got.cells.tobytes() == want.cells.tobytes(), (what, "cells")


@pytest.mark.parametrize("entry", ["integrate", "integrate_pair", "clearance", "clearance_batch", "simplify"])
def test_entries_that_return_host_results(H, ref_ctx, blocks, refs, delay, entry):
    """Called on freshly uploaded trees with the delay still pending on S (their first call builds the trees' caches behind it), at the
    depths tests/test_gpu_{integrate, integrate_pair, clearance, clearance_batch, simplify}.py use on synthetic trees; a Query is queued on
    S right behind them.  They return host structs, so they must wait: values only.  Catches: a level's kernels or read-back on stream 0
    or another stream (counts and sums read before they are written: another struct), a read-back without its wait, and for the Query
    behind them a context left on the wrong stream (P0's answer, the fill)."""
    call = _host_entries(H, blocks)[entry]
    want = call(ref_ctx, H.DeviceTree(ref_ctx, blocks["A"]), H.DeviceTree(ref_ctx, blocks["B"]))
    if entry == "simplify":
        assert want[0][1]["merges"] == 8 and want[1][1]["merges"] > 0 and want[1][1]["truncations"] > 0
    sets, qwant = refs("query", "A", N_TILES)
    with on_stream(H) as (ctx, S):
        tA, tB = H.DeviceTree(ctx, blocks["A"]), H.DeviceTree(ctx, blocks["B"])
        step = Step(H, ctx, ENTRIES["query"], tA, sets, N_TILES)
        with SO.quiet_host(), torch.cuda.stream(S):
            ev = delay.enqueue()
            pending_at_call = not ev.query()
            got = call(ctx, tA, tB)
            delay.enqueue()
            step.load()
            step.call()
            step.clone()
            step.overwrite()
        S.synchronize()
    assert pending_at_call
    _same_host_result(got, want, entry)
    step.check(qwant, ("the Query behind " + entry,))


def test_a_host_entry_waits_for_its_read_back(H, ref_ctx, blocks, delay):
    """hpsdf_query_host and hpsdf_query_gradient_host (host arrays in and out through the context's pinned scratch, as every *_host
    entry: csrc/host_call.hpp) with the delay pending on S, right after the same call for P0 -- whose answer is then what the pinned
    scratch still holds.  They must wait: values only.  Catches the wait in front of the copy out of the pinned scratch removed or
    made on another stream (P0's answer), and the copies or the launch on stream 0."""
    p0, p1 = (SO.points(np.random.default_rng(9200 + k), N_TILES)[0] for k in range(2))
    rt = H.DeviceTree(ref_ctx, blocks["deg4"])
    want = {"P0": (rt.query(p0),) + rt.query_with_gradient(p0), "P1": (rt.query(p1),) + rt.query_with_gradient(p1)}
    assert all(a.tobytes() != b.tobytes() for a, b in zip(want["P0"], want["P1"]))
    with on_stream(H) as (ctx, S):
        tree = H.DeviceTree(ctx, blocks["deg4"])
        got = {}
        for name, fn in (("query", lambda p: (tree.query(p),)), ("query_with_gradient", tree.query_with_gradient)):
            fn(p0)
            with SO.quiet_host(), torch.cuda.stream(S):
                ev = delay.enqueue()
                pending_at_call = not ev.query()
                got[name] = fn(p1)
            assert pending_at_call
    for name, outs, at in (("query", got["query"], 0), ("query_with_gradient", got["query_with_gradient"], 1)):
        for k, g in enumerate(outs):
            stale = "P0's answer: copied out before the stream had written it" if g.tobytes() == want["P0"][at + k].tobytes() else "neither P1's nor P0's"
            assert g.tobytes() == want["P1"][at + k].tobytes(), "%s: output %d is %s" % (name, k, stale)


# ------------------------------------------------------------------------------------------------------------ sequences on one context
def _sequence(H, ctx, refs, plan):
    """plan: [(tree name, the DeviceTree on ctx, n, seed)] -> the steps and what each must return"""
    steps, wants = [], []
    for name, tree, n, seed in plan:
        sets, want = refs("query", name, n, seed)
        steps.append(Step(H, ctx, ENTRIES["query"], tree, sets, n))
        wants.append(want)
    return steps, wants


def _run_sequence(S, delay, steps):
    """the delay, then load / call / clone for every step, then every overwrite: one stream, no host wait of the test's"""
    with torch.cuda.stream(S):
        ev = delay.enqueue()
        for st in steps:
            st.load()
            st.call()
            st.clone()
        pending = not ev.query()
        for st in steps:
            st.overwrite()
    S.synchronize()
    return pending


def _back_to_back(H, ctx, refs, blocks, big, other):
    tb, to = H.DeviceTree(ctx, blocks[big]), H.DeviceTree(ctx, blocks[other])
    return _sequence(H, ctx, refs, [(big, tb, N_FEW, 1), (big, tb, N_MANY, 2), (big, tb, N_FEW, 3), (other, to, N_TILES, 4)])


def test_back_to_back_queries_grow_the_scratch(H, blocks, refs, delay):
    """Query at 200, 300 000 and 200 points on the degree-12 tree, three output buffers, then 3 000 points on another tree: the second
    call needs longer deferred lists than the first allocated, while the first call's kernels are still queued behind the delay.  No
    no-wait assertion: growing the scratch frees device memory, which waits for the device (the header says so).  Catches: scratch
    freed or replaced under a queued call without that wait (a mixture in the earlier outputs), lists sized for another call, a call
    of the sequence on another stream (P0's answer, the fill)."""
    with on_stream(H) as (ctx, S):
        steps, wants = _back_to_back(H, ctx, refs, blocks, "deg12", "deg4")
        with SO.quiet_host():
            pending = _run_sequence(S, delay, steps)
    print("the delay was still running after the four calls:", pending)
    for k, (st, want) in enumerate(zip(steps, wants)):
        st.check(want, ("back to back", k, st.n))


@pytest.mark.parametrize("start", ["caller", "owned"])
def test_stream_change(H, blocks, refs, delay, start):
    """The delay and a 300 000-point Query on S1, hpsdf_ctx_set_stream(S2), a 3 000-point Query of the same degree-12 tree on S2 whose
    inputs were copied in on S1 BEFORE the change: the header promises that what the context queues after set_stream runs behind
    everything queued on the old stream by then, on the scratch the two calls share.  From a caller's stream the change must not wait on
    the host; from the library-owned stream it synchronises and destroys it.  Catches set_stream ordering nothing (the second Query
    runs at once on S2: P0's answer), a launch left on the old stream, and a host wait in the caller-to-caller change."""
    big_sets, big_want = refs("query", "deg12", N_MANY, 2)
    small_sets, small_want = refs("query", "deg12", N_TILES, 5)
    with on_stream(H, start) as (ctx, S1):
        S2 = torch.cuda.Stream()
        tree = H.DeviceTree(ctx, blocks["deg12"])
        big = Step(H, ctx, ENTRIES["query"], tree, big_sets, N_MANY)
        small = Step(H, ctx, ENTRIES["query"], tree, small_sets, N_TILES)
        with SO.quiet_host(), torch.cuda.stream(S1):
            ev = delay.enqueue()
            big.load()
            small.load()
            big.call()
            big.clone()
            big.overwrite()
        ctx.set_stream(S2.cuda_stream)
        pending = not ev.query()
        with torch.cuda.stream(S2):
            small.call()
            small.clone()
            small.overwrite()
        if start == "caller":
            S1.synchronize()                                                     # (the owned stream is gone: set_stream waited for it)
        S2.synchronize()
    big.check(big_want, ("stream change", start, "the Query on the old stream"))
    small.check(small_want, ("stream change", start, "the Query on the new stream"))
    if start == "caller":
        assert pending, "hpsdf_ctx_set_stream waited on the host between two caller streams"


def test_setting_the_stream_a_context_already_has(H, blocks, refs, delay):
    """hpsdf_ctx_set_stream with the context's own stream, as hpsdf_ctx_stream returned it: nothing changes -- the stream is not
    destroyed under the context, and the next call still runs on it in order.  Catches the owned stream destroyed and then used."""
    sets, want = refs("query", "deg12", N_TILES)
    with on_stream(H, "owned") as (ctx, S):
        ctx.set_stream(S.cuda_stream)
        assert H.lib().hpsdf_ctx_stream(ctx.handle) == S.cuda_stream
        step, pending = run_pattern(H, ctx, S, delay, ENTRIES["query"], H.DeviceTree(ctx, blocks["deg12"]), sets, N_TILES)
    step.check(want, ("the same stream set again",))
    assert pending, NO_WAIT


def test_two_contexts_two_threads(H, blocks, refs, delay):
    """Two contexts on two caller streams, each driven by its own Python thread through the back-to-back sequence on its own trees, at
    once.  (The header does not say that two contexts may share one uploaded tree, so they do not.)  Catches state that should be a
    context's own being shared: the deferred lists, a process-wide stream, launch arguments kept in globals (a mixture, or the other
    thread's answers)."""
    with on_stream(H) as (ctx0, S0), on_stream(H) as (ctx1, S1):
        plans = [_back_to_back(H, ctx0, refs, blocks, "deg12", "deg4"), _back_to_back(H, ctx1, refs, blocks, "deg12b", "inline")]
        torch.cuda.synchronize()
        gate, errors = threading.Barrier(2), []

        def drive(S, steps):
            try:
                gate.wait(30)
                _run_sequence(S, delay, steps)
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        threads = [threading.Thread(target=drive, args=(S, plan[0])) for S, plan in ((S0, plans[0]), (S1, plans[1]))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
    for who, (steps, wants) in enumerate(plans):
        for k, (st, want) in enumerate(zip(steps, wants)):
            st.check(want, ("thread", who, "call", k, st.n))


def test_create_ahead_of_query(H, ref_ctx, delay):
    """hpsdf_create of a small analytic field with the delay pending on the caller's stream, the upload of its block, and a Query of
    the new tree queued right behind.  Create returns a host block, so it waits: values only, for both.  Catches a build step or
    read-back on stream 0 or a stream that does not follow S (another block), the build's workspace left in use for the Query, a
    Query on another stream (P0's answer, the fill)."""
    cfg = H.make_config(1e-4)
    want_blk = H.create_block(ref_ctx, cfg, H.Field.sphere(), 1024)[0]
    sets = three_sets(ENTRIES["query"].make, N_TILES, 9100)
    want = synchronised(H, ref_ctx, ENTRIES["query"], H.DeviceTree(ref_ctx, want_blk), sets, N_TILES)
    with on_stream(H) as (ctx, S):
        step = Step(H, ctx, ENTRIES["query"], None, sets, N_TILES)
        with SO.quiet_host(), torch.cuda.stream(S):
            ev = delay.enqueue()
            pending_at_call = not ev.query()
            blk = H.create_block(ctx, cfg, H.Field.sphere(), 1024)[0]
            step.obj = H.DeviceTree(ctx, blk)
            delay.enqueue()
            step.load()
            step.call()
            step.clone()
            step.overwrite()
        S.synchronize()
    assert pending_at_call
    assert blk == want_blk, "the block built behind the delay differs from a default context's"
    step.check(want, ("the Query behind Create",))
