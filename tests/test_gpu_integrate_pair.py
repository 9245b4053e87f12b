"""IntegratePair on the GPU: the kernels (integrate_pair.hip) and the _host entry against the device-free entry byte for byte -- the degree
classes of both trees, an anisotropic root on each side, a deep chain as B, the smallest A, lists of 256 and 264 cells, one tree against
itself, max_leaves = 1, built trees --, repeatability, the cell limit, a non-finite B, the argument checks on the context entries, and a
C++ caller of the drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import integrate_reference as IR
from conftest import ROOT
from helpers import deep_chain_block, synthetic_block
from test_gpu_integrate import CASES, SYNTHETIC_MAX_CELLS, assert_same
from test_gpu_query_gradient import _built
from test_hiprec_cpu import ROOTS, _with_root
from test_integrate_cpu import assert_native_equals, parse_native, synthetic_iso
from test_integrate_pair_cpu import OPS, general_pose

DEGREES = {3: [3, 2, 1, 0, 3, 3, 2, 1], 5: [5, 4, 3, 2, 1, 0, 5, 4], 12: [12, 7, 3, 2, 9, 0, 5, 6]}


def check_pair(H, ctx, A, B, op, pose, iso_a, iso_b, D, q, max_cells, max_leaves, what, trees=None):
    """device and host entries against the block entry, with and without the cells -> the block entry's result"""
    want = H.integrate_pair_block(A, B, op, pose, iso_a, iso_b, D, q, max_cells, max_leaves, cells=True)
    tA, tB = trees or (H.DeviceTree(ctx, A), H.DeviceTree(ctx, B))
    args = (op, pose, iso_a, iso_b, D, q, max_cells, max_leaves)
    assert_same(tA.integrate_pair(tB, *args, cells=True), want, what + ("device",))
    assert_same(tA.integrate_pair(tB, *args), want, what + ("device, no cells",))
    assert_same(tA.integrate_pair(tB, *args, cells=True, host=True), want, what + ("host",))
    if trees is None:
        tA.close(), tB.close()
    return want


def synthetic_pair(rng, class_a, class_b, root_a="unit", root_b="unit"):
    A = synthetic_block(rng, DEGREES[class_a], 2, *ROOTS[root_a])
    B = synthetic_block(rng, DEGREES[class_b], 2, *ROOTS[root_b])
    return A, B


def pose_between(H, A, B, rng):
    """a general pose that carries the middle of A's root near the middle of B's, scaled so that the two roots cut through each other"""
    import hiprec as R
    a, b = R.Block(A), R.Block(B)
    ca, sa = 0.5 * (a.root_min + a.root_max).astype(np.float64), (a.root_max - a.root_min).astype(np.float64)
    cb, sb = 0.5 * (b.root_min + b.root_max).astype(np.float64), (b.root_max - b.root_min).astype(np.float64)
    M = general_pose(H).reshape(3, 4)[:, :3] * (0.8 * sb[:, None] / sa[None, :])
    return H.pose(M, cb + 0.2 * sb * rng.uniform(-1, 1, 3) - M @ ca)


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [(3, 12), (12, 3), (5, 5), (3, 3)])
def test_device_and_host_equal_block_entry_byte_for_byte_synthetic_pairs(H, ctx, classes):
    rng = np.random.default_rng(1301 + 13 * classes[0] + classes[1])
    statuses, decided = set(), 0
    for root_a, root_b in (("unit", "unit"), ("aniso", "cube"), ("cube", "aniso")):
        A, B = synthetic_pair(rng, *classes, root_a, root_b)
        tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
        assert (tA.info()["max_degree"], tB.info()["max_degree"]) == classes
        pose = pose_between(H, A, B, rng)
        iso_a, iso_b = synthetic_iso(H, A), synthetic_iso(H, B)
        for op in OPS:
            for D, q in CASES:
                want = check_pair(H, ctx, A, B, op, pose, iso_a, iso_b, D, q, SYNTHETIC_MAX_CELLS, 256, (classes, root_a, op, D, q), (tA, tB))
                statuses.add(want.status)
                decided += want.cells_inside + want.cells_outside
        tA.close(), tB.close()
    assert statuses == {H.INTEGRATE_OK, H.INTEGRATE_CELL_LIMIT} and decided > 100, (statuses, decided)


@pytest.mark.gpu
def test_a_deep_chain_the_smallest_tree_one_tree_twice_and_one_leaf_a_walk(H, ctx):
    rng = np.random.default_rng(1321)
    A = synthetic_block(rng, DEGREES[5], 2)
    deep = deep_chain_block(rng)                                                 # the walk's stack reaches its last level
    iso_a, iso_deep = synthetic_iso(H, A), synthetic_iso(H, deep)
    pose = general_pose(H, (0.1, 0.05, 0.12))
    for op in OPS:
        check_pair(H, ctx, A, deep, op, pose, iso_a, iso_deep, 4, 2, SYNTHETIC_MAX_CELLS, 4096, ("deep B", op))
        check_pair(H, ctx, deep, A, op, pose, iso_deep, iso_a, 4, 2, SYNTHETIC_MAX_CELLS, 256, ("deep A", op))
    small = synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)                    # list 0 has 8 cells
    want = check_pair(H, ctx, small, A, 0, pose, synthetic_iso(H, small), iso_a, 0, 1, 8, 256, ("smallest",))
    assert len(want.cells) == 8
    tree = H.DeviceTree(ctx, A)                                                  # tA == tB under a pose
    for op in OPS:
        check_pair(H, ctx, A, A, op, pose, iso_a, iso_a, 4, 2, SYNTHETIC_MAX_CELLS, 256, ("A against itself", op), (tree, tree))
    tree.close()
    wide = check_pair(H, ctx, A, deep, 0, pose, iso_a, iso_deep, 4, 2, SYNTHETIC_MAX_CELLS, 1, ("max_leaves 1",))
    free = H.integrate_pair_block(A, deep, 0, pose, iso_a, iso_deep, 4, 2, SYNTHETIC_MAX_CELLS, 4096)
    assert wide.unit_volume_hi - wide.unit_volume_lo >= free.unit_volume_hi - free.unit_volume_lo


@pytest.mark.gpu
def test_lists_of_256_and_264_cells(H, ctx):
    """A list of at most 256 cells is one workgroup's row, 264 cells put 8 rows into a second workgroup (test_gpu_integrate.py has why
    257 cannot exist).  The isos were found through the block entry; the lengths are asserted here."""
    A = synthetic_block(np.random.default_rng(601), [3, 2, 1, 0, 3, 3, 2, 1], 2)
    B = synthetic_block(np.random.default_rng(607), [5, 4, 3, 2, 1, 0, 5, 4], 2)
    pose = general_pose(H, (0.05, -0.1, 0.08))
    iso_b = 29.705282267224813
    for op, iso_a, length in ((0, -22.404590411791396, 256), (0, -17.967917385316582, 264), (1, 26.055856367823544, 256),
                              (1, 20.905639244020822, 264), (2, -31.90259535216186, 256), (2, -22.404590411791396, 264)):
        want = check_pair(H, ctx, A, B, op, pose, iso_a, iso_b, 3, 2, 1 << 24, 256, ("shape", op, length))
        assert IR.list_lengths(A, want)[-1] == length and max(IR.list_lengths(A, want)) == length


BUILT_POSE_T = (0.6, 0.3, 0.3)   # union3's root [-0.5, 0.5]^3 lands across sphere075's surface and across the low faces of its root


@pytest.mark.gpu
def test_built_trees_repeat_calls_a_second_handle_and_the_cell_limit(H, ctx):
    A, B = _built(H, ctx, "union3_1e-5"), _built(H, ctx, "sphere075_1e-6")
    pose = general_pose(H, BUILT_POSE_T)
    tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    first = None
    for op in OPS:
        want = check_pair(H, ctx, A, B, op, pose, 1e-5, 1e-6, 7, 2, 1 << 24, 256, ("built", op), (tA, tB))
        assert want.status == H.INTEGRATE_OK and want.unit_volume_lo <= want.unit_volume <= want.unit_volume_hi
        assert want.cells_inside > 100 and want.cells_outside > 100
        print("op %d: volume in [%.6f, %.6f], %d cells, %d evaluations" % (op, want.volume_lo, want.volume_hi, len(want.cells), want.evaluations))
        first = first or want
    args = (0, pose, 1e-5, 1e-6, 7, 2)
    assert first.overlapping and not first.disjoint
    other = tA.integrate_pair(tB, 2, pose, 0.013, 0.0, 5, 4, cells=True)             # another call in between
    assert other.raw != first.raw
    assert_same(tA.integrate_pair(tB, *args, cells=True), first, ("a repeat call",))
    t2, t3 = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)                             # second handles: their own list 0 and constants
    assert_same(t2.integrate_pair(t3, *args, cells=True), first, ("second handles",))
    t2.close(), t3.close()
    lengths = IR.list_lengths(A, first)
    limit = lengths[2] - 1                                                       # list 2 does not fit: level 1 is final
    want = H.integrate_pair_block(A, B, *args, limit, cells=True)
    assert want.status == H.INTEGRATE_CELL_LIMIT and want.levels == 1
    assert_same(tA.integrate_pair(tB, *args, limit, cells=True), want, ("cell limit, device",))
    assert_same(tA.integrate_pair(tB, *args, limit, cells=True, host=True), want, ("cell limit, host",))
    assert_same(tA.integrate_pair(tB, *args, cells=True), first, ("after the limit",))
    tA.close(), tB.close()
    one, two = H.Octree(), H.Octree()
    one.FromMemoryBlock(A), two.FromMemoryBlock(B)
    assert_same(one.IntegratePair(two, *args, cells=True), first, ("Octree.IntegratePair",))


@pytest.mark.gpu
def test_a_non_finite_coefficient_in_b_on_the_device(H, ctx):
    import hiprec as R
    good = synthetic_block(np.random.default_rng(1327), DEGREES[3], 2)
    Bk = R.Block(good)
    leaf = int(Bk.descend(np.array([[0.25, 0.25, 0.25]]))[0])
    raw = bytearray(good)
    at = 8 + 8 * int(Bk.start[leaf])
    raw[at:at + 8] = np.array([np.inf]).tobytes()
    iso = synthetic_iso(H, good)
    want = H.integrate_pair_block(good, bytes(raw), 1, None, iso, iso, 4, 2, cells=True)
    assert want.status == H.INTEGRATE_NOT_FINITE
    tA, tB = H.DeviceTree(ctx, good), H.DeviceTree(ctx, bytes(raw))
    for host in (False, True):
        got = tA.integrate_pair(tB, 1, None, iso, iso, 4, 2, cells=True, host=host)
        assert got.status == H.INTEGRATE_NOT_FINITE and len(got.cells) == 0 and got.raw == want.raw
    assert tA.integrate_pair(tA, 1, None, iso, iso, 4, 2).status == H.INTEGRATE_OK
    tA.close(), tB.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_context_usable(H, ctx):
    blk = synthetic_block(np.random.default_rng(1361), [2, 1, 0, 2, 2, 1, 2, 0], 1)
    tree = H.DeviceTree(ctx, blk)
    L = H.lib()
    st = H.hpsdf_integral()
    C.memset(C.byref(st), 7, C.sizeof(st))
    seven = bytes(st)
    ptr, count = C.c_void_p(77), C.c_uint64(77)
    untouched = lambda: bytes(st) == seven and ptr.value == 77 and count.value == 77
    identity = H.pose()
    bad_pose = identity.copy()
    bad_pose[3] = np.inf
    for fn in (L.hpsdf_integrate_pair_device, L.hpsdf_integrate_pair_host):
        def call(ta=tree.handle, tb=tree.handle, op=0, pose=identity, iso_a=0.0, iso_b=0.0, depth=4, samples=2, max_cells=4096, max_leaves=256,
                 out=C.byref(st), c=C.byref(ptr), n=C.byref(count), cx=ctx.handle):
            return fn(cx, ta, tb, op, pose.ctypes.data_as(C.c_void_p) if pose is not None else None, iso_a, iso_b, depth, samples, max_cells,
                      max_leaves, out, c, n)
        refused = lambda **kw: call(**kw) == H.ERR_INVALID_ARGUMENT and untouched()
        assert refused(iso_a=float("nan")) and refused(iso_b=float("inf")) and refused(pose=bad_pose) and refused(pose=None)
        assert refused(op=3) and refused(depth=16) and refused(samples=3) and refused(max_cells=7) and refused(max_cells=(1 << 28) + 1)
        assert refused(max_leaves=0) and refused(max_leaves=65536)
        assert refused(out=None) and refused(n=None) and refused(c=None) and refused(ta=None) and refused(tb=None)
        assert call(cx=None) == H.ERR_NO_DEVICE and untouched()
    want = H.integrate_pair_block(blk, blk, 2, general_pose(H), 0.0, 0.1, 5, 2, cells=True)   # the context and the tree still answer
    assert_same(tree.integrate_pair(tree, 2, general_pose(H), 0.0, 0.1, 5, 2, cells=True), want, ("after the refusals",))
    assert_same(tree.integrate_pair(tree, 2, general_pose(H), 0.0, 0.1, 5, 2, cells=True, host=True), want, ("after the refusals, host",))
    tree.close()


def build_pair_caller(H, tmp_path):
    exe = str(tmp_path / "integrate_pair_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "integrate_pair_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/integrate_pair_caller.cpp through include/hpsdf_octree.hpp: the structs and the cells it prints are the Python binding's."""
    A, B = _built(H, ctx, "union3_1e-5"), _built(H, ctx, "sphere075_1e-6")
    pose = general_pose(H, BUILT_POSE_T)
    exe = build_pair_caller(H, tmp_path)
    (tmp_path / "a.bin").write_bytes(A)
    (tmp_path / "b.bin").write_bytes(B)
    (tmp_path / "pose.bin").write_bytes(pose.tobytes())
    r = subprocess.run([exe, str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "pose.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = parse_native(r.stdout)
    assert_native_equals(got["a"], H.integrate_pair_block(A, A, 0), "defaults: A against itself under the identity")
    assert len(got["a"][2]) == 0
    assert_native_equals(got["b"], H.integrate_pair_block(A, B, 1, pose, 0.013, 0.0, 6, 4, 1 << 24, 64, cells=True), "b")
    limited = H.integrate_pair_block(A, B, 2, pose, 0.0, 0.0, 7, 2, 512, 256, cells=True)
    assert limited.status == H.INTEGRATE_CELL_LIMIT
    assert_native_equals(got["c"], limited, "c")
