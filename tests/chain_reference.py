"""The running total of Create's stop rule (Octree.cpp:253-290) as a plain loop, the ways a device chain could get it wrong, and the
operand lists that tell them apart.  Python floats and numpy only: nothing here calls the product.

The reference is `sequential`: t = total0; for every operand in order, t = t + x -- one IEEE double addition after the other.  The three
models are what a chain that adds four operands an instruction would compute if the instruction did not round after every term in
order (`grouped`, `exact4`), or flushed subnormals (`flushed`); `reversed` is the wrong lane order.  Every family comes from a fixed
seed, as a Case: the operands, and a round-0 rendering of the same operands -- nine error slots a job and the batch's earlier errors,
with errs[9 k] - batch_err[k] == ops[k] bit for bit, so that both operand sources of the device chain have ONE reference."""
import math
import struct
from collections import namedtuple

import numpy as np

# the borders of the remainder (n & 3), the step tail (n / 4 mod 16), the even and odd batch counts and the 2048-operand chunks
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 60, 63, 64, 65, 67, 127, 128, 129, 131, 191, 192, 193, 255, 256, 2044, 2045, 2047, 2048, 2049, 2051, 2052, 2112,
           4095, 4096, 4097, 6147)
LONG_LENGTHS = LENGTHS + (4099,)  # mixed and errors: two chunks and a remainder of 3 as well
SEPARATING = 8                    # from this length on a family must separate the models (a 7-operand mixed list does not)
DBL_MIN = 2.2250738585072014e-308
HALF_ULP = 2.0 ** -53             # half an ulp of 1.0

Case = namedtuple("Case", "family name total0 ops errs batch_err")


def bits(x):
    return struct.pack("<d", float(x))


def same(a, b):
    """Equal bit for bit; a NaN equals a NaN whatever its payload (the only relaxation: signed zeros and infinities compare by bits)."""
    a, b = float(a), float(b)
    return (a != a and b != b) or bits(a) == bits(b)


def _floats(ops):
    return np.asarray(ops, np.float64).tolist()


def sequential(total0, ops):
    t = float(total0)
    for x in _floats(ops):
        t = t + x
    return np.float64(t)


def round0_operands(errs, batch_err):
    """What round 0 adds: float64(errs[9 k]) - float64(batch_err[k]), formed first."""
    errs, batch_err = np.asarray(errs, np.float64), np.asarray(batch_err, np.float64)
    assert errs.size == 9 * batch_err.size
    with np.errstate(all="ignore"):
        return errs[0::9] - batch_err


def sequential_round0(total0, errs, batch_err):
    return sequential(total0, round0_operands(errs, batch_err))


def reversed_order(total0, ops):
    return sequential(total0, _floats(ops)[::-1])


def grouped(total0, ops):
    """t + ((a0 + a1) + (a2 + a3)) per step of four; the remainder one by one."""
    x, t = _floats(ops), float(total0)
    n4 = len(x) & ~3
    for i in range(0, n4, 4):
        t = t + ((x[i] + x[i + 1]) + (x[i + 2] + x[i + 3]))
    for v in x[n4:]:
        t = t + v
    return np.float64(t)


def exact4(total0, ops):
    """Each step of four rounded once; the remainder one by one."""
    x, t = _floats(ops), float(total0)
    n4 = len(x) & ~3
    for i in range(0, n4, 4):
        t = math.fsum([t] + x[i:i + 4])
    for v in x[n4:]:
        t = t + v
    return np.float64(t)


def _flush(v):
    return math.copysign(0.0, v) if 0.0 < abs(v) < DBL_MIN else v


def flushed(total0, ops):
    """Subnormal operands and results replaced by a zero of their sign."""
    t = _flush(float(total0))
    for x in _floats(ops):
        t = _flush(t + _flush(x))
    return np.float64(t)


# ---------------------------------------------------------------------------------------------------------------- round-0 rendering
def split(ops, rng):
    """(errs[9 n], batch_err[n]) with errs[9 k] - batch_err[k] == ops[k] bit for bit: x = x/2 - (-x/2) where halving is exact, else
    2x - x, else x - 0 (which keeps a zero's sign, an infinity and a NaN).  The eight other slots of a job hold numbers that no sum
    wants: a chain that reads a wrong slot is far off."""
    x = np.asarray(ops, np.float64)
    n = x.size
    errs = np.ldexp(1.0 + rng.random(9 * n), 40)
    e, b = x.copy(), np.zeros(n)
    with np.errstate(all="ignore"):
        for ce, cb in ((2 * x, x), (x / 2, -x / 2)):  # (the later candidate wins where it is exact)
            d = ce - cb
            good = ((d.view(np.uint64) == x.view(np.uint64)) | (np.isnan(d) & np.isnan(x))) & (np.isinf(ce) <= np.isinf(x))
            e, b = np.where(good, ce, e), np.where(good, cb, b)
    errs[0::9] = e
    batch_err = b
    assert all(same(a, b) for a, b in zip(round0_operands(errs, batch_err).tolist(), x.tolist()))
    return errs, batch_err


def _case(family, name, total0, ops, rng, errs=None, batch_err=None):
    ops = np.asarray(ops, np.float64)
    if errs is None:
        errs, batch_err = split(ops, rng)
    return Case(family, name, float(total0), ops, errs, batch_err)


# ---------------------------------------------------------------------------------------------------------------- the families
def mixed_operands(rng, n):
    """Mantissa in [1, 2), exponent uniform in -30 .. 29, random sign (tools/mfma_chain_lab.hip's rnd())."""
    m = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52
    return np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0) * np.ldexp(m, rng.integers(-30, 30, n).astype(np.int32))


def separates(case, reversal=True):
    """The condition on a list: its sequential sum differs in its bits from the grouped one, from the one rounded once a step and
    (reversal) from the reversed list's."""
    want = sequential(case.total0, case.ops)
    wrong = [grouped(case.total0, case.ops), exact4(case.total0, case.ops)] + ([reversed_order(case.total0, case.ops)] if reversal else [])
    return not any(same(want, w) for w in wrong)


def _first_separating(make, seed, n):
    """A random list need not separate the models (the last bits of two different roundings can meet again): the list of n operands is
    the one from the first of the seeds seed + n, seed + n + 10000, ... that does.  tests/test_chain_cpu.py asserts the outcome."""
    for attempt in range(64):
        case = make(np.random.default_rng(seed + n + 10000 * attempt), n)
        if n < SEPARATING or separates(case):
            return case
    raise AssertionError("no separating list of %d operands" % n)


def _mixed(rng, n):
    return _case("mixed", "mixed", mixed_operands(rng, 1)[0], mixed_operands(rng, n), rng)


def _errors(rng, n):
    new_err, old_err = rng.random(n) * 1e-6, rng.random(n) * 1e-5
    errs = np.ldexp(1.0 + rng.random(9 * n), 40)
    errs[0::9] = new_err
    return _case("errors", "errors", rng.random() * 1e-2, new_err - old_err, rng, errs, old_err)


def mixed(n):
    return _first_separating(_mixed, 260601, n)


def errors(n):
    """u 1e-6 - v 1e-5, the shape of newErr - initialErr: the round-0 rendering IS the two terms, and the subtraction rounds."""
    return _first_separating(_errors, 260602, n)


def ties(n):
    """Half-ulp operands: from 1.0 the sequential sum drops every one (ties to even), from 1 + 2^-52 it does not; and runs of five
    +2^-53, five -2^-53 taking turns (runs, so that a step of four is not always two of each)."""
    rng = np.random.default_rng(260603 + n)
    runs = np.where((np.arange(n) // 5) % 2 == 0, HALF_ULP, -HALF_ULP)
    return [_case("ties", "dropped", 1.0, np.full(n, HALF_ULP), rng), _case("ties", "kept", 1.0 + 2.0 ** -52, np.full(n, HALF_ULP), rng),
            _case("ties", "runs", 1.0, runs, rng)]


def cancellation(n):
    """1e16, 1, -1e16, 1, ...: whole periods only (n a multiple of four) -- cut inside a period, the list ends on the large term and
    what the models disagree about is absorbed: it separates nothing there."""
    assert n % 4 == 0
    rng = np.random.default_rng(260604 + n)
    return _case("cancellation", "cancellation", 0.0, np.tile([1e16, 1.0, -1e16, 1.0], n // 4), rng)


CANCELLATION_LENGTHS = tuple(n for n in LENGTHS if n % 4 == 0)
SUBNORMALS = (4.94e-324, -4.94e-324, 1e-310, -3e-315, 2.2250738585072009e-308, -2.2250738585072014e-308)  # tools/mfma_chain_lab.hip's


def subnormal(n):
    """From DBL_MIN, operands at and below the normal range: additions are exact while the total stays below 2 DBL_MIN, so order hardly
    matters -- flushing does."""
    rng = np.random.default_rng(260605 + n)
    return _case("subnormal", "subnormal", DBL_MIN, rng.choice(np.array(SUBNORMALS), n), rng)


def special(n):
    """Signed zeros, overflow, inf - inf and a NaN: n operands each (n >= 3 for the ones that need a place in the middle)."""
    rng = np.random.default_rng(260606 + n)
    mid = n // 2
    out = [_case("special", "minus zeros", -0.0, np.full(n, -0.0), rng)]
    if n >= 1:
        z = np.full(n, -0.0)
        z[mid] = 0.0
        out.append(_case("special", "one plus zero", -0.0, z, rng))
        v = mixed_operands(rng, n)
        v[mid] = 1.7e308  # (the total overflows here, in the middle, and stays +inf)
        out.append(_case("special", "overflow", 1.7e308, v, rng))
    if n >= 3:
        v = mixed_operands(rng, n)
        v[mid - 1], v[mid] = np.inf, -np.inf
        out.append(_case("special", "inf then -inf", 1.0, v, rng))
        v = mixed_operands(rng, n)
        v[mid] = np.nan
        out.append(_case("special", "nan", 1.0, v, rng))
    return out


SPECIAL_LENGTHS = (1, 3, 5, 64, 67, 2049, 6147)  # a place in every code path: remainder, step tail, batches, second chunk, fourth chunk


# ---------------------------------------------------------------------------------------------------------------- the position family
POSITION_CONSTANT = 0x1B6DB6DB6DB6DB  # odd, 53 bits: every operand has its last mantissa bit set


def position(n):
    """Two lists in which every place counts.
    magnitude: operand k is 2^(k mod 40) times an odd 53-bit constant (scaled into [1, 2) first).  Neighbours differ in magnitude and no
      operand is a sum of others, so a dropped or a doubled operand changes the total.  A SWAP of neighbours it cannot show wherever the
      total dominates both: with t a multiple of its ulp u and no change of exponent, (t + a) + b = t + rnd_u(a) + rnd_u(b) = (t + b) + a
      in any IEEE arithmetic -- and from the second cycle of forty on the total does dominate.
    parity: 2^-53 and 2^-52 taking turns, from 1 + 2^-52 (odd) -- half an ulp and one ulp.  The half ulp is dropped from an even total and carries
      an odd one up (ties to even); the whole ulp flips the parity.  Swapping two neighbours changes which of the two happens, and the
      totals differ from there to the end by two ulps of the same parity: a swap anywhere shows, as does a drop (a doubled half ulp does not: the second one meets an
      even total -- duplicates are the magnitude list's).
    position_perturbations and tests/test_chain_cpu.py try all of it: proved, not assumed."""
    rng = np.random.default_rng(260607 + n)
    ops = np.ldexp(float(POSITION_CONSTANT), (np.arange(n) % 40 - 52).astype(np.int32))
    turns = np.where(np.arange(n) % 2 == 0, HALF_ULP, 2 * HALF_ULP)
    return [_case("position", "magnitude", float(POSITION_CONSTANT) * 2.0 ** -60, ops, rng), _case("position", "parity", 1.0 + 2.0 ** -52, turns, rng)]


def border_places(n):
    """The places of an n-operand list next to a border of the chain: the ends, the steps of four, the batches of 64, the chunks."""
    near = set()
    for b in (0, 4, 64, 128, 2048, 4096, 6144, n & ~3, n & ~63, n & ~2047, n):
        near.update(range(b - 3, b + 3))
    return sorted(k for k in near if 0 <= k < n)


def position_perturbations(n):
    """(list, what, place, total0, operands) at the border places: every single-operand drop (both lists), duplicate (the magnitude
    list) and swap with the next operand (the parity list)."""
    for case in position(n):
        ops = case.ops
        for k in border_places(n):
            yield case.name, "drop", k, case.total0, np.delete(ops, k)
            if case.name == "magnitude":
                yield case.name, "duplicate", k, case.total0, np.insert(ops, k, ops[k])
            elif k + 1 < n:
                s = ops.copy()
                s[k], s[k + 1] = s[k + 1], s[k]
                yield case.name, "swap", k, case.total0, s


# ---------------------------------------------------------------------------------------------------------------- what the tests walk
def cases(family):
    """Every Case of a family, at the lengths it is defined for."""
    if family == "mixed":
        return [mixed(n) for n in LONG_LENGTHS]
    if family == "errors":
        return [errors(n) for n in LONG_LENGTHS]
    if family == "ties":
        return [c for n in LENGTHS for c in ties(n)]
    if family == "cancellation":
        return [cancellation(n) for n in CANCELLATION_LENGTHS]
    if family == "subnormal":
        return [subnormal(n) for n in LENGTHS]
    if family == "special":
        return [c for n in SPECIAL_LENGTHS for c in special(n)]
    if family == "position":
        return [c for n in LENGTHS for c in position(n)]
    raise KeyError(family)


FAMILIES = ("mixed", "errors", "ties", "cancellation", "subnormal", "special", "position")
