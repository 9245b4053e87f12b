"""The running total of Create's stop rule on the GPU -- frRunChain itself, through hpsdf_selftest_running_total -- against the plain
sequential sum of tests/chain_reference.py, bit for bit: four additions an instruction on the matrix pipe must round after every term,
in operand order, keep subnormals and signed zeros, and lose or double no operand at any border of the remainder, the step tail, the
batches and the 2048-operand chunks; from both operand sources (the dense list of later rounds, round 0's errs[9 k] - batchErr[k]) and
with both wave populations (sixteen waves, thirteen).  tests/test_chain_cpu.py shows that these operands tell a wrong chain from a
right one.  A failure here means that Create's total, hence the round a build stops in, hence the block's bytes, are not the
reference's."""
import ctypes as C

import numpy as np
import pytest

import chain_reference as R

SOURCES = ("ops", "round0")
POPULATIONS = ("sixteen waves", "thirteen waves")


def run_chain(H, ctx, case, source, population):
    pop = H.CHAIN_ALL_WAVES if population == "sixteen waves" else H.CHAIN_THIRTEEN_WAVES
    if source == "ops":
        return H.selftest_running_total(ctx, case.total0, ops=case.ops, population=pop)
    return H.selftest_running_total(ctx, case.total0, errs=case.errs, batch_err=case.batch_err, population=pop)


@pytest.fixture(scope="module")
def reference():
    """family -> [(case, the sequential sum)]: computed once, shared by every test below, never written to."""
    out = {}
    for family in R.FAMILIES:
        out[family] = [(c, R.sequential(c.total0, c.ops)) for c in R.cases(family)]
        for c, _ in out[family]:
            for a in (c.ops, c.errs, c.batch_err):
                a.setflags(write=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("population", POPULATIONS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_chain_gives_the_sequential_sum_bit_for_bit(H, ctx, reference, family, source, population):
    wrong = []
    for case, want in reference[family]:
        got = run_chain(H, ctx, case, source, population)
        if not R.same(got, want):  # (a NaN for a NaN, whatever the payload: the only relaxation; zeros and infinities by their bits)
            models = {m: R.same(got, f(case.total0, case.ops)) for m, f in (("grouped", R.grouped), ("reversed", R.reversed_order), ("flushed", R.flushed))}
            wrong.append((case.name, len(case.ops), float(got).hex(), float(want).hex(), [m for m, hit in models.items() if hit]))
    print("%s, %s, %s: %d lists compared, %d differ" % (family, source, population, len(reference[family]), len(wrong)))
    assert not wrong, wrong[:8]


@pytest.mark.gpu
def test_repeated_and_interleaved_calls_give_the_same_bits(H, ctx, reference):
    """The chain keeps nothing between calls: the same list gives the same bits again, also after a longer and after a shorter list
    have been through the same LDS buffer halves."""
    pick = {n: (c, w) for c, w in reference["mixed"] for n in [len(c.ops)]}
    order = (6147, 5, 2049, 6147, 0, 2048, 5, 4099, 3, 2049, 6147)
    seen = {}
    for n in order:
        case, want = pick[n]
        for source in SOURCES:
            for population in POPULATIONS:
                got = run_chain(H, ctx, case, source, population)
                assert R.same(got, want), (n, source, population)
                assert seen.setdefault((n, source, population), R.bits(got)) == R.bits(got)
    assert len(seen) == 7 * 4


@pytest.mark.gpu
def test_a_call_between_two_creates_leaves_the_second_block_equal(H, ctx, reference):
    """The entry works in the host calls' scratch: Create's frontier workspace -- header, operand list, error slots -- is not touched."""
    cfg, field = H.make_config(1e-7), H.Field.sphere()   # (seven rounds of 256 jobs)
    first, st1 = H.create_block(ctx, cfg, field, 256)
    assert st1["device_frontier"] == 1 and st1["rounds"] >= 3   # (later rounds' dense operand list and round 0's error slots were both in use)
    for family in ("mixed", "special"):
        for case, want in reference[family]:
            if len(case.ops) in (3, 2049, 6147):
                for source in SOURCES:
                    assert R.same(run_chain(H, ctx, case, source, "thirteen waves"), want)
    second, st2 = H.create_block(ctx, cfg, field, 256)
    assert second == first and np.float64(st2["total_error"]).tobytes() == np.float64(st1["total_error"]).tobytes()
    assert {k: st1[k] for k in ("rounds", "jobs", "n_nodes", "n_coeffs")} == {k: st2[k] for k in ("rounds", "jobs", "n_nodes", "n_coeffs")}


@pytest.mark.gpu
def test_argument_checks_leave_the_context_usable(H, ctx, reference):
    L = H.lib()
    out = C.c_double(77.0)
    ops, errs, batch = np.arange(8.0), np.arange(72.0), np.arange(8.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(cx=ctx.handle, total0=1.0, n=8, source=H.CHAIN_OPS, population=H.CHAIN_ALL_WAVES, o=ops, e=errs, b=batch, res=C.byref(out)):
        return L.hpsdf_selftest_running_total(cx, total0, n, source, population, ptr(o), ptr(e), ptr(b), res)
    untouched = lambda: out.value == 77.0
    refused = lambda **kw: call(**kw) == H.ERR_INVALID_ARGUMENT and untouched() and bool(L.hpsdf_last_error())
    assert refused(n=1 << 24) and refused(n=(1 << 24) + 5) and refused(n=1 << 40)
    assert refused(source=2) and refused(source=-1) and refused(population=2) and refused(population=-1)
    assert refused(o=None) and refused(source=H.CHAIN_ROUND0, e=None) and refused(source=H.CHAIN_ROUND0, b=None) and refused(res=None)
    assert call(cx=None) == H.ERR_NO_DEVICE and untouched()
    # what is not an error: no operands at all (the arrays may be NULL then), and the other source's arrays missing
    for source in (H.CHAIN_OPS, H.CHAIN_ROUND0):
        for t0 in (-0.0, 2.5, float("inf")):
            out.value = 77.0
            assert call(total0=t0, n=0, source=source, o=None, e=None, b=None) == 0 and R.bits(out.value) == R.bits(t0)
    assert call(e=None, b=None) == 0 and out.value == 1.0 + 28.0
    assert call(source=H.CHAIN_ROUND0, o=None) == 0 and out.value == 1.0 + sum(9.0 * k - k for k in range(8))
    case, want = reference["errors"][-1]                                       # the context still answers
    assert R.same(run_chain(H, ctx, case, "round0", "sixteen waves"), want)
    with pytest.raises(H.HpsdfError) as ei:
        H.selftest_running_total(ctx, 0.0, ops=np.zeros(8), population=7)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT
