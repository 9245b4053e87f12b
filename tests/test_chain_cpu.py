"""The inputs of tests/test_gpu_running_total.py can tell a wrong chain from a right one: conditions on tests/chain_reference.py's operand
families, checked on the CPU -- were one of them to fail, the GPU test would pass a chain it ought to catch.  And the new entry's
declaration, binding and export."""
import os
import re

import numpy as np
import pytest

import chain_reference as R
from conftest import ROOT


def test_the_models_are_what_they_say():
    h = R.HALF_ULP
    assert R.sequential(1.0, [h] * 4) == 1.0                                   # every half ulp dropped
    assert R.grouped(1.0, [h] * 4) == R.exact4(1.0, [h] * 4) == 1.0 + 4 * h   # ... kept by a chain that adds them up first
    assert R.sequential(1.0 + 2 * h, [h]) == 1.0 + 4 * h                       # ties to even: up from an odd total
    assert R.reversed_order(0.0, [1e16, 1.0, -1e16]) == 0.0 and R.sequential(0.0, [-1e16, 1.0, 1e16]) == 0.0
    assert R.sequential(0.0, [1e16, -1e16, 1.0]) == 1.0
    assert R.flushed(R.DBL_MIN, [-4.94e-324]) == R.DBL_MIN and R.sequential(R.DBL_MIN, [-4.94e-324]) == 2.225073858507201e-308  # (a subnormal)
    assert R.bits(R.flushed(R.DBL_MIN, [-3e-315, -1.5 * R.DBL_MIN])) == R.bits(-0.0)  # (the operand is dropped, the result flushed)
    assert R.bits(R.flushed(-0.0, [-1e-310])) == R.bits(-0.0)
    assert R.same(np.nan, -np.nan) and not R.same(0.0, -0.0) and not R.same(np.inf, -np.inf) and R.same(np.inf, np.inf)
    assert R.grouped(0.0, [1.0, 2.0, 3.0, 4.0, 5.0]) == R.exact4(0.0, [1.0, 2.0, 3.0, 4.0, 5.0]) == 15.0  # (the remainder is added too)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_both_operand_sources_have_one_reference(family):
    """errs[9 k] - batch_err[k] is ops[k] bit for bit (a NaN for a NaN), and the eight other slots of a job are not operands."""
    lengths = set()
    for c in R.cases(family):
        n = len(c.ops)
        lengths.add(n)
        assert c.errs.shape == (9 * n,) and c.batch_err.shape == (n,) and c.ops.dtype == c.errs.dtype == c.batch_err.dtype == np.float64
        got = R.round0_operands(c.errs, c.batch_err)
        assert all(R.same(a, b) for a, b in zip(got.tolist(), c.ops.tolist())), (family, c.name, n)
        assert R.same(R.sequential(c.total0, c.ops), R.sequential_round0(c.total0, c.errs, c.batch_err))
        others = np.delete(c.errs, np.arange(0, 9 * n, 9))
        assert np.all(others >= 2.0 ** 40)
    if family in ("mixed", "errors"):
        assert lengths == set(R.LENGTHS) | {4099} and 6147 in lengths
    elif family == "cancellation":
        assert lengths == {n for n in R.LENGTHS if n % 4 == 0}
    elif family == "special":
        assert lengths == set(R.SPECIAL_LENGTHS)
    else:
        assert lengths == set(R.LENGTHS)
    if family == "errors":   # the subtraction is a real one there: it rounds
        c = R.errors(2051)
        assert np.all(c.batch_err > 0) and np.any(c.errs[0::9] - c.ops != c.batch_err)
    elif family not in ("special", "subnormal"):  # ... and elsewhere both terms are there
        assert all(np.all(c.batch_err != 0) for c in R.cases(family))


@pytest.mark.parametrize("family", ["mixed", "errors", "ties", "cancellation"])
def test_the_sequential_sum_differs_from_every_wrong_model(family):
    """From eight operands on: not the grouped sum, not the sum rounded once a step; mixed, errors and cancellation: not the reversed
    list's either (half-ulp operands of one size are the same list backwards)."""
    seen = 0
    for c in R.cases(family):
        if len(c.ops) < R.SEPARATING:
            continue
        want = R.sequential(c.total0, c.ops)
        assert not R.same(want, R.grouped(c.total0, c.ops)), (family, c.name, len(c.ops), "grouped")
        assert not R.same(want, R.exact4(c.total0, c.ops)), (family, c.name, len(c.ops), "exact4")
        if family != "ties":
            assert not R.same(want, R.reversed_order(c.total0, c.ops)), (family, c.name, len(c.ops), "reversed")
        seen += 1
    assert seen == {"mixed": 28, "errors": 28, "ties": 81, "cancellation": 11}[family]


def test_ties_are_dropped_from_one_and_kept_from_the_next_double():
    for n in R.LENGTHS:
        dropped, kept, runs = R.ties(n)
        assert R.sequential(dropped.total0, dropped.ops) == 1.0
        assert R.sequential(kept.total0, kept.ops) == (1.0 + 2.0 ** -51 if n else 1.0 + 2.0 ** -52)
        assert set(np.abs(runs.ops).tolist()) <= {R.HALF_ULP} and (n < 6 or (runs.ops > 0).any() and (runs.ops < 0).any())


def test_subnormals_survive_only_without_flushing():
    """Additions of subnormals are exact, so order hardly matters down there: what the list must catch is a flush to zero."""
    for c in R.cases("subnormal"):
        n = len(c.ops)
        want = R.sequential(c.total0, c.ops)
        if n:
            assert not R.same(want, R.flushed(c.total0, c.ops)), n
            assert set(c.ops.tolist()) <= set(R.SUBNORMALS) and abs(float(want)) < 1e-300
    assert len(set(R.subnormal(2048).ops.tolist())) == len(R.SUBNORMALS) == 6


def test_special_values_give_what_ieee_says():
    seen = set()
    for c in R.cases("special"):
        want, n = R.sequential(c.total0, c.ops), len(c.ops)
        seen.add(c.name)
        if c.name == "minus zeros":
            assert R.bits(want) == R.bits(-0.0)
        elif c.name == "one plus zero":
            assert R.bits(want) == R.bits(0.0) and np.count_nonzero(np.signbit(c.ops)) == n - 1
        elif c.name == "overflow":
            assert R.bits(want) == R.bits(np.inf) and np.all(np.isfinite(c.ops))
        elif c.name == "inf then -inf":
            k = int(np.flatnonzero(np.isinf(c.ops))[0])
            assert np.isnan(want) and c.ops[k] == np.inf and c.ops[k + 1] == -np.inf and np.isinf(R.sequential(c.total0, c.ops[:k + 1]))
        else:
            assert c.name == "nan" and np.isnan(want) and np.count_nonzero(np.isnan(c.ops)) == 1 and 0 < np.flatnonzero(np.isnan(c.ops))[0] < n - 1
    assert seen == {"minus zeros", "one plus zero", "overflow", "inf then -inf", "nan"}


def test_every_place_of_the_position_lists_counts():
    """Every single-operand drop (both lists), duplicate (the magnitude list) and swap of neighbours (the parity list) next to an end, a
    step, a batch or a chunk border changes the total's bits -- at every length.  (Why the magnitude list cannot show a swap, and the
    parity list not a duplicate: chain_reference.position.)"""
    tried = {}
    for n in R.LENGTHS:
        want = {c.name: R.sequential(c.total0, c.ops) for c in R.position(n)}
        places = R.border_places(n)
        assert all(0 <= k < n for k in places) and (n < 2052 or {2046, 2047, 2048, 2049} <= set(places)) and (n < 68 or {62, 63, 64, 65} <= set(places))
        for name, what, k, total0, ops in R.position_perturbations(n):
            assert len(ops) == n + {"drop": -1, "duplicate": 1, "swap": 0}[what]
            assert not R.same(want[name], R.sequential(total0, ops)), (name, what, n, k)
            tried[name, what] = tried.get((name, what), 0) + 1
    assert set(tried) == {("magnitude", "drop"), ("magnitude", "duplicate"), ("parity", "drop"), ("parity", "swap")} and min(tried.values()) > 500, tried
    ops = R.position(6147)[0].ops
    assert np.array_equal(ops[:40] * 2.0 ** 52, float(R.POSITION_CONSTANT) * 2.0 ** np.arange(40)) and R.POSITION_CONSTANT % 2 == 1
    assert np.array_equal(ops[40:80], ops[:40]) and R.POSITION_CONSTANT.bit_length() == 53


def test_a_swap_under_a_dominating_total_is_invisible_to_any_sum():
    """The reason the magnitude list leaves swaps to the parity list: it is arithmetic, not a gap in the list."""
    c = R.position(131)[0]
    for k in (62, 63, 64, 127, 128):
        s = c.ops.copy()
        s[k], s[k + 1] = s[k + 1], s[k]
        if k % 40 < 30:
            assert R.same(R.sequential(c.total0, c.ops), R.sequential(c.total0, s)), k


def test_new_symbols_are_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_selftest_running_total"}
    assert new <= declared and declared == set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    m = re.search(r"enum \{ HPSDF_CHAIN_OPS = (\d), HPSDF_CHAIN_ROUND0 = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.CHAIN_OPS, H.CHAIN_ROUND0) == (0, 1)
    m = re.search(r"enum \{ HPSDF_CHAIN_ALL_WAVES = (\d), HPSDF_CHAIN_THIRTEEN_WAVES = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.CHAIN_ALL_WAVES, H.CHAIN_THIRTEEN_WAVES) == (0, 1)
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == 4 == H.ABI_VERSION == H.lib().hpsdf_abi_version()
    assert callable(H.selftest_running_total)
    # the entry runs the chain Create runs: the kernel calls frRunChain, and there is one frRunChain
    src = open(os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "csrc", "frontier.hip")).read()
    kernel = src[src.index("void fr_running_total_kernel("):]
    kernel = kernel[:kernel.index("\n}\n")]
    assert "frRunChain(d, L, total0, n, round0 != 0)" in kernel and "mfma" not in kernel
    assert len(re.findall(r"^__device__ double frRunChain\(", src, re.M)) == 1 and src.count("frRunChain(d, L,") == 3
