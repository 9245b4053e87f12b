"""Integrate on the GPU: the kernels (integrate.hip) and the _host entry against the device-free entry byte for byte -- every degree class,
an anisotropic root, a deep chain, built trees, the smallest tree, the reduction's one-, two- and three-pass shapes --, repeatability,
the cell limit, the argument checks on the context entries, and a C++ caller of the drop-in."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import integrate_reference as IR
from helpers import synthetic_block
from test_gpu_query_gradient import _built, _trees
from test_integrate_cpu import assert_native_equals, build_caller, parse_native, synthetic_iso

CASES = ((0, 1), (4, 2), (7, 4))
SYNTHETIC_MAX_CELLS = 1 << 13      # random polynomial trees are undecided almost everywhere: their lists are capped (CELL_LIMIT at depth 7)


def assert_same(got, want, what):
    assert got.raw == want.raw, (what, "struct", got, want)
    if got.cells is not None:                                                    # (a call made without the cells: the struct alone)
        assert got.cells.dtype == want.cells.dtype and got.cells.shape == want.cells.shape, (what, got.cells.shape, want.cells.shape)
        assert got.cells.tobytes() == want.cells.tobytes(), (what, "cells", int((got.cells != want.cells).sum()))


def check_tree(H, ctx, blk, iso, D, q, max_cells, what):
    """device and host entries against the block entry, with and without the cells -> the block entry's result"""
    want = H.integrate_block(blk, iso, D, q, max_cells, cells=True)
    tree = H.DeviceTree(ctx, blk)
    assert_same(tree.integrate(iso, D, q, max_cells, cells=True), want, what + ("device",))
    assert_same(tree.integrate(iso, D, q, max_cells), want, what + ("device, no cells",))
    assert_same(tree.integrate(iso, D, q, max_cells, cells=True, host=True), want, what + ("host",))
    tree.close()
    return want


@pytest.mark.gpu
def test_device_and_host_equal_block_entry_byte_for_byte_synthetic_trees(H, ctx):
    rng = np.random.default_rng(571)
    degrees, statuses, smallest = set(), set(), False
    for name, blk in _trees(rng):
        tree = H.DeviceTree(ctx, blk)
        degrees.add(tree.info()["max_degree"])
        tree.close()
        iso = synthetic_iso(H, blk)
        for D, q in CASES:
            want = check_tree(H, ctx, blk, iso, D, q, SYNTHETIC_MAX_CELLS, (name, D, q))
            statuses.add(want.status)
            if D == 0 and len(want.cells) == 8:                                 # a tree whose list 0 has 8 cells: the smallest case
                smallest = True
    assert {2, 3, 5, 12} <= degrees and statuses == {H.INTEGRATE_OK, H.INTEGRATE_CELL_LIMIT} and smallest, (degrees, statuses, smallest)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["union3_1e-5", "sphere075_1e-6"])
def test_device_and_host_equal_block_entry_byte_for_byte_built_trees(H, ctx, case):
    blk = _built(H, ctx, case)
    for iso in (0.0, 0.013):
        for D, q in CASES:
            want = check_tree(H, ctx, blk, iso, D, q, 1 << 24, (case, iso, D, q))
            assert want.status == H.INTEGRATE_OK
            assert want.unit_volume_lo <= want.unit_volume <= want.unit_volume_hi
    print("%s: D=7 volume in [%.6f, %.6f], %d cells, %d evaluations" % (case, want.volume_lo, want.volume_hi, len(want.cells), want.evaluations))


@pytest.mark.gpu
def test_the_reductions_one_two_and_three_pass_shapes(H, ctx):
    """A list of at most 256 cells is one workgroup's row; more need a second pass over the workgroups' rows, more than 65 536 a third.
    The lengths are found on the CPU through the block entry and asserted here.  A list of exactly 257 cells cannot exist: list 0 holds
    8 + 7 m leaves (257 = 5 mod 7) and every later list a multiple of 8; 264 is the smallest length above 256 a refined list can have,
    and it puts 8 rows into the second workgroup."""
    blk = synthetic_block(np.random.default_rng(601), [3, 2, 1, 0, 3, 3, 2, 1], 2)
    for iso, length in ((-31.745702743530273, 256), (-22.646072387695312, 264)):
        want = check_tree(H, ctx, blk, iso, 3, 2, 1 << 24, ("shape", length))
        assert IR.list_lengths(blk, want)[-1] == length and max(IR.list_lengths(blk, want)) == length
    big = _built(H, ctx, "union3_1e-5")
    want = check_tree(H, ctx, big, 0.0, 8, 1, 1 << 24, ("shape", "three passes"))
    lengths = IR.list_lengths(big, want)
    assert max(lengths) > 65536 and min(lengths) > 256, lengths
    print("list lengths of union3 @ 1e-5 at depth 8:", lengths)


@pytest.mark.gpu
def test_a_second_call_gives_the_same_bytes_and_the_cell_limit_is_the_hosts(H, ctx):
    blk = _built(H, ctx, "union3_1e-5")
    tree = H.DeviceTree(ctx, blk)
    first = tree.integrate(0.0, 6, 2, cells=True)
    assert_same(tree.integrate(0.0, 6, 2, cells=True), first, ("second call",))
    other = tree.integrate(0.013, 5, 4, cells=True)                              # another call in between
    assert other.raw != first.raw
    assert_same(tree.integrate(0.0, 6, 2, cells=True), first, ("third call",))
    t2 = H.DeviceTree(ctx, blk)                                                  # a second handle: its own list 0 and constants
    assert_same(t2.integrate(0.0, 6, 2, cells=True), first, ("a second handle",))
    t2.close()
    lengths = IR.list_lengths(blk, first)
    limit = lengths[2] - 1                                                       # list 2 does not fit: level 1 is final
    want = H.integrate_block(blk, 0.0, 6, 2, limit, cells=True)
    assert want.status == H.INTEGRATE_CELL_LIMIT and want.levels == 1
    assert_same(tree.integrate(0.0, 6, 2, limit, cells=True), want, ("cell limit, device",))
    assert_same(tree.integrate(0.0, 6, 2, limit, cells=True, host=True), want, ("cell limit, host",))
    assert_same(tree.integrate(0.0, 6, 2, cells=True), first, ("after the limit",))
    tree.close()
    one = H.Octree()
    one.FromMemoryBlock(blk)
    assert_same(one.Integrate(0.0, 6, 2, cells=True), first, ("Octree.Integrate",))
    assert np.array_equal(H.cells_to_boxes(one, first.cells[:50]), H.cells_to_boxes(blk, first.cells[:50]))


@pytest.mark.gpu
def test_a_non_finite_coefficient_on_the_device(H, ctx):
    import hiprec as R
    blk = synthetic_block(np.random.default_rng(577), [3, 2, 1, 0, 3, 3, 2, 1], 2)
    B = R.Block(blk)
    leaf = int(B.descend(np.array([[0.25, 0.25, 0.25]]))[0])
    raw = bytearray(blk)
    at = 8 + 8 * int(B.start[leaf])
    raw[at:at + 8] = np.array([np.inf]).tobytes()
    want = H.integrate_block(bytes(raw), 0.0, 4, 2, cells=True)
    assert want.status == H.INTEGRATE_NOT_FINITE
    tree = H.DeviceTree(ctx, bytes(raw))
    got = tree.integrate(0.0, 4, 2, cells=True)
    assert got.status == H.INTEGRATE_NOT_FINITE and len(got.cells) == 0
    assert got.raw == want.raw
    tree.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_context_usable(H, ctx):
    blk = synthetic_block(np.random.default_rng(587), [2, 1, 0, 2, 2, 1, 2, 0], 1)
    tree = H.DeviceTree(ctx, blk)
    L = H.lib()
    st = H.hpsdf_integral()
    C.memset(C.byref(st), 7, C.sizeof(st))
    seven = bytes(st)
    ptr, count = C.c_void_p(77), C.c_uint64(77)
    untouched = lambda: bytes(st) == seven and ptr.value == 77 and count.value == 77
    for fn in (L.hpsdf_integrate_device, L.hpsdf_integrate_host):
        call = lambda tr=tree.handle, iso=0.0, depth=4, samples=2, max_cells=4096, out=C.byref(st), c=C.byref(ptr), n=C.byref(count), cx=ctx.handle: \
            fn(cx, tr, iso, depth, samples, max_cells, out, c, n)
        assert call(iso=float("nan")) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(iso=float("inf")) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(depth=16) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(samples=3) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(max_cells=7) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(max_cells=(1 << 28) + 1) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(out=None) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(n=None) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(c=None) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(tr=None) == H.ERR_INVALID_ARGUMENT and untouched()
        assert call(cx=None) == H.ERR_NO_DEVICE and untouched()
    want = H.integrate_block(blk, 0.0, 5, 2, cells=True)                        # the context and the tree still answer
    assert_same(tree.integrate(0.0, 5, 2, cells=True), want, ("after the refusals",))
    assert_same(tree.integrate(0.0, 5, 2, cells=True, host=True), want, ("after the refusals, host",))
    tree.close()


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/integrate_caller.cpp through include/hpsdf_octree.hpp: the struct and the cells it prints are the Python binding's."""
    from helpers import product_field
    blk = H.create_block(ctx, H.make_config(1e-5), product_field(H, "union3"), 1024)[0]
    exe = build_caller(H, tmp_path)
    (tmp_path / "blk.bin").write_bytes(blk)
    r = subprocess.run([exe, str(tmp_path / "blk.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = parse_native(r.stdout)
    assert_native_equals(got["a"], H.integrate_block(blk), "defaults")
    assert len(got["a"][2]) == 0
    assert_native_equals(got["b"], H.integrate_block(blk, 0.013, 6, 4, 1 << 24, cells=True), "b")
    limited = H.integrate_block(blk, 0.0, 7, 2, 512, cells=True)
    assert limited.status == H.INTEGRATE_CELL_LIMIT
    assert_native_equals(got["c"], limited, "c")
