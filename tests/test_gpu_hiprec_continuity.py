"""The continuity post-process on the device -- continuity_asm.hip's matrix, cg.hip's solve with both of its SpMV kernels, and
Create with continuity.enforce -- against the extended-precision reference (tests/hiprec_continuity.py).  The parity tests pin the
device to the host and the host to the oracle; these pin all three to the face integrals and to the true residual."""
import numpy as np
import pytest

import hiprec as R
import hiprec_continuity as RC
from test_hiprec_continuity_cpu import (BUILT, STRENGTH, check_capped, check_matrix, check_solve, multiple_of_256,
                                        ref_of, root_leaf_block, synthetic_case, tol_of, xstar)

pytestmark = pytest.mark.gpu

K_CG_CHUNK, K_CG_ROW_TAIL = 256, 1024        # csrc/launch.hpp: kCgChunk, kCgRowTail
MATRIX_CASES = ("eight", "mixed", "chain4", "chain10", "built")
SOLVE_CASES = ("eight", "chain4", "chain10", "built", "mixed", "x256")
# The largest observed figure / bound per check, printed at the end of the module (the slack the bounds leave).
WORST = {}


def _worst(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def blocks(H, ctx):
    out = {name: synthetic_case(name) for name in ("eight", "mixed", "chain4", "chain10", "x256")}
    cfg = H.make_config(BUILT[1], continuity=False)
    cfg.continuity_strength = STRENGTH
    out["built"], _ = H.create_block(ctx, cfg, H.Field.union3(), BUILT[2])
    yield out
    if WORST:
        print("\nlargest figure / bound per check: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize("name", MATRIX_CASES)
def test_device_matrix_within_the_entry_bounds(H, ctx, blocks, name):
    """hpsdf_continuity_matrix_device: pair counts, numeric-pair counts, pattern and every value against M* -- conforming faces
    only (eight leaves), degrees 0..12 with rows of 1303 entries (mixed), depth differences up to 3 and up to 9 across one face
    (the chains), and a built tree with both kinds of face."""
    blk = blocks[name]
    ref = ref_of(name, blk)
    assert ref.n_undecided <= 1e-3 * ref.n_contrib
    rp, ci, v, st = H.continuity_matrix_device(ctx, blk)
    _worst("matrix", check_matrix(ref, rp, ci, v, st, "device " + name))
    assert st["nnz"] == len(v)
    if name == "chain10":
        b = R.Block(blk)
        assert int(b.depth[b.leaves()].max()) == 10 and int(b.depth[b.leaves()].min()) == 1
    if name == "built":
        assert ref.n_numeric > 1000 and ref.n_analytic > 1000


@pytest.mark.parametrize("which", ["default", "tight"])
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_device_solve_against_the_true_residual(H, ctx, blocks, name, which):
    """hpsdf_continuity_post_process_device: the assertions of the host solve (tests/test_hiprec_continuity_cpu.py), at the
    default tolerance and at TIGHT_TOL, the drift term below 1e-2 of tol ||b|| at both.  Eight leaves:
    n = 383, one full 256-row chunk and a 127-row tail; x256: n = 512, two full chunks; the mixed tree: 18 chunks and a longest row
    of 1303 > kCgRowTail, which sends the solve to the row-owned SpMV -- every other case stays below and takes the entry-cut one."""
    blk = blocks[name]
    tol = tol_of(name, which)
    ref = ref_of(name, blk)
    star = xstar(name, ref, blk) if ref.n <= 4500 else None
    out, st = H.continuity_post_process(blk, tol, 0, ctx=ctx)
    got = check_solve(ref, blk, out, st, tol, "device " + name, star)
    for k, v in got.items():
        _worst("solve " + k, v)
    assert st["iterations"] > 0 and out[8 + 8 * ref.n:] == blk[8 + 8 * ref.n:]
    longest = int(np.diff(H.continuity_matrix_device(ctx, blk)[0].astype(np.int64)).max())
    assert longest == ref.longest_row
    assert (longest > K_CG_ROW_TAIL) == (name == "mixed")
    if name == "eight":
        assert ref.n == 383 == K_CG_CHUNK + 127
    if name == "x256":
        assert multiple_of_256() == [0, 0, 0, 0, 0, 0, 9, 10] and ref.n == 2 * K_CG_CHUNK
    if name == "mixed":
        assert longest == 1303 and (ref.n + K_CG_CHUNK - 1) // K_CG_CHUNK == 18


@pytest.mark.parametrize("name", ("eight", "mixed", "chain4", "chain10", "x256"))
def test_device_capped_runs_are_conjugate_gradient_iterates(H, ctx, blocks, name):
    """max_iter in {1, 2, 3, 5} at tol 1e-30 on the device: see check_capped (tests/test_hiprec_continuity_cpu.py)."""
    blk = blocks[name]
    ref = ref_of(name, blk)
    worst = check_capped(ref, blk, lambda k: H.continuity_post_process(blk, 1e-30, k, ctx=ctx), "device " + name, xstar(name, ref, blk))
    _worst("iterate", worst)


def test_a_root_that_is_a_leaf_on_the_device(H, ctx):
    """No pairs, an empty matrix, and the solve's single step onto c: the device path gives what the host path gives."""
    blk = RC.with_strength(root_leaf_block(np.random.default_rng(9), 5), STRENGTH)
    rp, ci, v, st = H.continuity_matrix_device(ctx, blk)
    assert st["n_pairs"] == 0 and st["nnz"] == 0 and len(v) == 0 and not rp.any()
    host, sh = H.continuity_post_process(blk)
    dev, sd = H.continuity_post_process(blk, ctx=ctx)
    assert dev == host and sd["iterations"] == sh["iterations"] == 0
    c, x = R.Block(blk).coeffs, R.Block(dev).coeffs
    assert (np.abs(x - c) <= 16 * R.U * np.abs(c)).all()


def test_create_with_continuity_solves_the_reference_system(H, ctx, blocks):
    """hpsdf_create with continuity.enforce on the built tree: the same tree as the continuity-free build, its coefficients x
    satisfy A* x = lambda c (c the continuity-free build's) at the default tolerance, and continuity_last_stats() carries the
    reference's pair counts and jump energies."""
    blk0 = blocks["built"]
    ref = ref_of("built", blk0)
    cfg = H.make_config(BUILT[1], continuity=True)
    cfg.continuity_strength = STRENGTH
    blk, _ = H.create_block(ctx, cfg, H.Field.union3(), BUILT[2])
    cs = H.continuity_last_stats()
    b0 = bytearray(blk0)
    b0[-80 + 16] = 1                                       # continuity.enforce of the serialised config
    assert blk[8 + 8 * ref.n:] == bytes(b0)[8 + 8 * ref.n:]
    assert (cs["n_pairs"], cs["n_pairs_analytic"], cs["n_pairs_numeric"], cs["nnz"]) == (ref.n_pairs, ref.n_analytic, ref.n_numeric, ref.nnz)
    got = check_solve(ref, blk0, blk, cs, 0.0, "create", None)
    for k, v in got.items():
        _worst("create " + k, v)
    assert cs["iterations"] > 0 and cs["jump_after"] < cs["jump_before"]
