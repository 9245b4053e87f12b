"""Pins the oracle's constant tables: against the reference's own headers (compiled where they lie,
oracle/_ref) when the checkout is present, else against their values stored in tests/golden/ref_tables.npz,
and against the committed hashes of those tables always."""
import os

import numpy as np

from conftest import GOLDEN, bits
from helpers import sha

NAMES = ("roots", "weights", "normalised_lengths", "recurrence", "coeff_count", "basis_index", "sum_to_n")


def stored_ref_tables():
    """The reference's tables and scalars as tests/golden/make_golden.py read them from oracle/_ref."""
    with np.load(os.path.join(GOLDEN, "ref_tables.npz")) as d:
        return {k: d[k] for k in d.files}


def test_oracle_tables_match_reference_headers_bitwise(O):
    ref = O.ref_tables() or stored_ref_tables()
    t = O.tables()
    for k in NAMES:
        assert np.array_equal(bits(t[k]), bits(ref[k])), k


def test_oracle_scalars_match_reference_headers(O):
    """Consts.h:7-8, Literals.h:3-13 and MemoryBlock.h:5-9 compiled where they lie: the limits, the widths of the
    reference's integer typedefs on this ABI ("u32" is 8 bytes) and EPSILON_F32 of the closest-point guards."""
    import ctypes as C
    want = [12, 10, 4, 8, 8, 8, 16, int(np.float32(0.000001).view(np.uint32))]
    got = (C.c_ulonglong * 8)()
    O.lib().ora_scalars(got)
    assert list(got) == want
    R = O.ref_tables_lib()
    if R is not None and hasattr(R, "ref_scalars"):
        ref = (C.c_ulonglong * 8)()
        R.ref_scalars(ref)
        ref = list(ref)
    else:
        ref = [int(x) for x in stored_ref_tables()["scalars"]]
    assert ref == want


def test_oracle_tables_match_committed_reference_hashes(O, golden):
    t = O.tables()
    for k in NAMES:
        assert sha(t[k]) == golden["tables"][k]["sha256"], k


def test_known_quirks(O, golden):
    t = O.tables()
    # Include/HP/Utility.h:87-106: the f64 evaluation truncates 84 to 83 for degree 6
    assert [int(x) for x in t["coeff_count"]] == [1, 4, 10, 20, 35, 56, 83, 120, 165, 220, 286, 364, 455]
    assert t["basis_index"][82:86].astype(int).tolist() == [[5, 1, 0], [6, 0, 0], [0, 0, 7], [0, 1, 6]]
    assert t["basis_index"][:12].astype(int).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 2], [0, 1, 1],
                                                          [0, 2, 0], [1, 0, 1], [1, 1, 0], [2, 0, 0], [0, 0, 3], [0, 1, 2]]
    # Legendre.h stores the 9-point rule's pairs as 3rd,4th,1st,2nd smallest |x|
    a = np.abs(t["roots"][36:45])
    assert a[0] == 0 and a[1] == a[2] and a[1] > a[5] and a[3] > a[1] and a[5] < a[7]
    assert np.allclose(a, golden["tables"]["spot"]["gl9_abs_order"], rtol=0, atol=0)


def test_gauss_legendre_rules_integrate(O):
    t = O.tables()
    for n in range(1, 65):
        s = n * (n - 1) // 2
        x, w = t["roots"][s:s + n], t["weights"][s:s + n]
        assert abs(w.sum() - 2.0) < 1e-14
        assert abs((w * x * x).sum() - (2.0 / 3.0 if n > 1 else 0.0)) < 1e-14
        assert np.array_equal(np.sort(np.abs(x[n % 2:]))[::2], np.sort(np.abs(x[n % 2:]))[1::2])  # exact +- pairs


def test_normalised_lengths_values(O):
    nl = O.tables()["normalised_lengths"]
    for i in range(13):
        for j in range(11):
            # Utility.h:25-35 is a 100-step Newton iteration, not a correctly rounded sqrt: some entries sit
            # 1 ulp off (e.g. [4][1]); the bit-exact pin is the reference-hash test above
            assert abs(nl[i, j] - np.sqrt((2 * i + 1) * 2.0 ** j)) <= 4.5e-16 * nl[i, j]
