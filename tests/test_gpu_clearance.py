"""Clearance on the GPU: the kernels (clearance.hip) and the _host entry against the device-free entry byte for byte, the struct and the
cells -- the degree classes of both trees on unit and anisotropic roots, a deep chain as B and as A, the smallest A, one tree against
itself, max_leaves = 1, lists of 256 and 264 cells, a constant B whose candidates all tie across workgroups, built trees --,
repeatability, the cell limit, a non-finite B, the argument checks on the context entries, and a C++ caller of the drop-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clearance_reference as CR
from conftest import ROOT
from helpers import deep_chain_block, synthetic_block
from test_clearance_cpu import parse_clearance_native
from test_gpu_integrate import assert_same
from test_gpu_integrate_pair import BUILT_POSE_T, DEGREES, pose_between, synthetic_pair
from test_gpu_query_gradient import _built
from test_integrate_cpu import synthetic_iso
from test_integrate_pair_cpu import constant_block, general_pose


def check_clearance(H, ctx, A, B, pose, iso_a, D, tol, max_cells, max_leaves, what, trees=None):
    """device and host entries against the block entry, with and without the cells -> the block entry's result"""
    want = H.clearance_block(A, B, pose, iso_a, D, tol, max_cells, max_leaves, cells=True)
    tA, tB = trees or (H.DeviceTree(ctx, A), H.DeviceTree(ctx, B))
    args = (pose, iso_a, D, tol, max_cells, max_leaves)
    assert_same(tA.clearance(tB, *args, cells=True), want, what + ("device",))
    assert_same(tA.clearance(tB, *args), want, what + ("device, no cells",))
    assert_same(tA.clearance(tB, *args, cells=True, host=True), want, what + ("host",))
    if trees is None:
        tA.close(), tB.close()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [(3, 12), (12, 3), (5, 5), (3, 3)])
def test_device_and_host_equal_block_entry_byte_for_byte_synthetic_pairs(H, ctx, classes):
    rng = np.random.default_rng(1501 + 13 * classes[0] + classes[1])
    statuses, pruned = set(), 0
    for root_a, root_b in (("unit", "unit"), ("aniso", "cube"), ("cube", "aniso")):
        A, B = synthetic_pair(rng, *classes, root_a, root_b)
        tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
        assert (tA.info()["max_degree"], tB.info()["max_degree"]) == classes
        pose = pose_between(H, A, B, rng)
        iso_a = synthetic_iso(H, A)
        for D, tol in ((0, 0.0), (3, 0.0), (5, 0.0), (5, 1e9)):
            want = check_clearance(H, ctx, A, B, pose, iso_a, D, tol, 1 << 13, 256, (classes, root_a, D, tol), (tA, tB))
            statuses.add(want.status)
            pruned += want.cells_pruned
            assert np.isfinite(want.hi)
        tA.close(), tB.close()
    assert {H.CLEARANCE_DEPTH, H.CLEARANCE_CONVERGED} <= statuses and pruned > 100, (statuses, pruned)


@pytest.mark.gpu
def test_a_deep_chain_the_smallest_tree_one_tree_twice_and_one_leaf_a_walk(H, ctx):
    rng = np.random.default_rng(1521)
    A = synthetic_block(rng, DEGREES[5], 2)
    deep = deep_chain_block(rng)                                                 # the walk's stack reaches its last level
    iso_a, iso_deep = synthetic_iso(H, A), synthetic_iso(H, deep)
    pose = general_pose(H, (0.1, 0.05, 0.12))
    check_clearance(H, ctx, A, deep, pose, iso_a, 4, 0.0, 1 << 13, 4096, ("deep B",))
    check_clearance(H, ctx, deep, A, pose, iso_deep, 4, 0.0, 1 << 13, 256, ("deep A",))
    small = synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)                    # list 0 has 8 cells
    want = check_clearance(H, ctx, small, A, pose, synthetic_iso(H, small), 0, 0.0, 8, 256, ("smallest",))
    assert want.cells_visited == 8 and want.levels == 0
    tree = H.DeviceTree(ctx, A)                                                  # tA == tB
    check_clearance(H, ctx, A, A, None, iso_a, 4, 0.0, 1 << 13, 256, ("A against itself, the identity",), (tree, tree))
    check_clearance(H, ctx, A, A, pose, iso_a, 4, 0.0, 1 << 13, 256, ("A against itself under a pose",), (tree, tree))
    tree.close()
    wide = check_clearance(H, ctx, A, deep, pose, iso_a, 4, 0.0, 1 << 13, 1, ("max_leaves 1",))
    free = H.clearance_block(A, deep, pose, iso_a, 4, 0.0, 1 << 13, 4096)
    assert wide.lo <= free.lo and wide.hi >= free.hi


@pytest.mark.gpu
def test_lists_of_256_and_264_cells(H, ctx):
    """A list of at most 256 cells is one workgroup's row of the two reductions, 264 cells put 8 lanes into a second workgroup (a list
    past list 0 is a multiple of 8 long: 257 cannot exist).  The isos were found through the block entry's rule: the replay of
    tests/clearance_reference.py over the 0.02 .. 0.98 quantiles of Query_A, in steps of 0.01, at D = 3; the first whose longest list had
    256 and 264 cells were kept.  The lengths are asserted here."""
    A = synthetic_block(np.random.default_rng(601), [3, 2, 1, 0, 3, 3, 2, 1], 2)
    B = synthetic_block(np.random.default_rng(607), [5, 4, 3, 2, 1, 0, 5, 4], 2)
    pose = general_pose(H, (0.05, -0.1, 0.08))
    for iso_a, length in ((-4.607380069522278, 256), (-3.775846687353257, 264)):
        want = check_clearance(H, ctx, A, B, pose, iso_a, 3, 0.0, 1 << 24, 256, ("shape", length))
        ref = CR.replay(H, A, B, pose, iso_a, 3)
        CR.assert_equal(want, ref, ("shape", length))
        assert max(ref["lengths"]) == length, ref["lengths"]


@pytest.mark.gpu
def test_every_candidate_ties_across_workgroups(H, ctx):
    """B constant: every candidate has the same vb, so the witness must be the candidate of the smallest pos of list 0 -- which here is
    longer than 256 cells, so the minimum crosses workgroups and a fold pass -- and no later level may replace it."""
    A = _built(H, ctx, "union3_1e-5")
    const = constant_block(0.75)
    tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, const)
    for D in (4, 5):
        want = check_clearance(H, ctx, A, const, None, 1e-5, D, 0.0, 1 << 24, 256, ("ties", D), (tA, tB))
        assert want.cells_visited > 256 and np.isfinite(want.hi)
        full = H.clearance_block(A, const, None, 1e300, 0, 1e300, cells=True)   # list 0 itself, in order
        boxes = H.cells_to_boxes(A, full.cells)
        centres = 0.5 * (boxes[:, :3] + boxes[:, 3:])
        first = int(np.nonzero(H.query_gradient_block(A, centres)[0] < 1e-5)[0][0])
        assert first > 256 or len(centres) > 256
        assert np.array_equal(want.point, centres[first]), (want.point, centres[first], first)
    tA.close(), tB.close()


@pytest.mark.gpu
def test_built_trees_repeat_calls_a_second_handle_and_the_cell_limit(H, ctx):
    A, B = _built(H, ctx, "union3_1e-5"), _built(H, ctx, "sphere075_1e-6")
    pose = general_pose(H, BUILT_POSE_T)
    tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    first = check_clearance(H, ctx, A, B, pose, 1e-5, 7, 0.0, 1 << 24, 256, ("built",), (tA, tB))
    assert first.status == H.CLEARANCE_DEPTH and first.lo <= first.hi < 1e-6 and first.cells_pruned > 100   # the solids interfere
    print("built: %r, gap %r, %d visited, %d outside A, %d pruned" % (first, first.gap(1e-6), first.cells_visited, first.cells_outside_a, first.cells_pruned))
    args = (pose, 1e-5, 7, 0.0)
    other = tA.clearance(tB, None, 0.013, 5, 1e-3, cells=True)                    # another call in between
    assert other.raw != first.raw
    assert_same(tA.clearance(tB, *args, cells=True), first, ("a repeat call",))
    t2, t3 = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)                          # second handles: their own list 0 and constants
    assert_same(t2.clearance(t3, *args, cells=True), first, ("second handles",))
    t2.close(), t3.close()
    limit = 64                                                                  # list 1 does not fit: level 0 is final
    want = H.clearance_block(A, B, *args, limit, cells=True)
    assert want.status == H.CLEARANCE_CELL_LIMIT and want.levels == 0 and want.lo <= first.lo and want.hi >= first.hi
    assert_same(tA.clearance(tB, *args, limit, cells=True), want, ("cell limit, device",))
    assert_same(tA.clearance(tB, *args, limit, cells=True, host=True), want, ("cell limit, host",))
    assert_same(tA.clearance(tB, *args, cells=True), first, ("after the limit",))
    conv = check_clearance(H, ctx, A, B, pose, 1e-5, 12, 0.05, 1 << 24, 256, ("converged",), (tA, tB))
    assert conv.status == H.CLEARANCE_CONVERGED and conv.hi - conv.lo <= 0.05
    tA.close(), tB.close()
    one, two = H.Octree(), H.Octree()
    one.FromMemoryBlock(A), two.FromMemoryBlock(B)
    assert_same(one.Clearance(two, *args, cells=True), first, ("Octree.Clearance",))


@pytest.mark.gpu
def test_a_non_finite_coefficient_in_b_on_the_device(H, ctx):
    import hiprec as R
    good = synthetic_block(np.random.default_rng(1527), DEGREES[3], 2)
    Bk = R.Block(good)
    leaf = int(Bk.descend(np.array([[0.25, 0.25, 0.25]]))[0])
    raw = bytearray(good)
    at = 8 + 8 * int(Bk.start[leaf])
    raw[at:at + 8] = np.array([np.inf]).tobytes()
    iso = synthetic_iso(H, good)
    want = H.clearance_block(good, bytes(raw), None, iso, 4, cells=True)
    assert want.status == H.CLEARANCE_NOT_FINITE
    tA, tB = H.DeviceTree(ctx, good), H.DeviceTree(ctx, bytes(raw))
    for host in (False, True):
        got = tA.clearance(tB, None, iso, 4, cells=True, host=host)
        assert got.status == H.CLEARANCE_NOT_FINITE and len(got.cells) == 0 and got.raw == want.raw
    assert tA.clearance(tA, None, iso, 4).status == H.CLEARANCE_DEPTH
    tA.close(), tB.close()


@pytest.mark.gpu
def test_argument_checks_leave_the_context_usable(H, ctx):
    blk = synthetic_block(np.random.default_rng(1561), [2, 1, 0, 2, 2, 1, 2, 0], 1)
    tree = H.DeviceTree(ctx, blk)
    L = H.lib()
    st = H.hpsdf_clearance()
    C.memset(C.byref(st), 7, C.sizeof(st))
    seven = bytes(st)
    ptr, count = C.c_void_p(77), C.c_uint64(77)
    untouched = lambda: bytes(st) == seven and ptr.value == 77 and count.value == 77
    identity = H.pose()
    bad_pose = identity.copy()
    bad_pose[3] = np.inf
    for fn in (L.hpsdf_clearance_device, L.hpsdf_clearance_host):
        def call(ta=tree.handle, tb=tree.handle, pose=identity, iso_a=0.0, depth=4, tol=0.0, max_cells=4096, max_leaves=256, out=C.byref(st),
                 c=C.byref(ptr), n=C.byref(count), cx=ctx.handle):
            return fn(cx, ta, tb, pose.ctypes.data_as(C.c_void_p) if pose is not None else None, iso_a, depth, tol, max_cells, max_leaves, out, c, n)
        refused = lambda **kw: call(**kw) == H.ERR_INVALID_ARGUMENT and untouched()
        assert refused(iso_a=float("nan")) and refused(pose=bad_pose) and refused(pose=None)
        assert refused(tol=-1.0) and refused(tol=float("inf")) and refused(tol=float("nan"))
        assert refused(depth=16) and refused(max_cells=7) and refused(max_cells=(1 << 28) + 1)
        assert refused(max_leaves=0) and refused(max_leaves=65536)
        assert refused(out=None) and refused(n=None) and refused(c=None) and refused(ta=None) and refused(tb=None)
        assert call(cx=None) == H.ERR_NO_DEVICE and untouched()
    want = H.clearance_block(blk, blk, general_pose(H), 0.1, 5, cells=True)      # the context and the tree still answer
    assert_same(tree.clearance(tree, general_pose(H), 0.1, 5, cells=True), want, ("after the refusals",))
    assert_same(tree.clearance(tree, general_pose(H), 0.1, 5, cells=True, host=True), want, ("after the refusals, host",))
    tree.close()


def build_clearance_caller(H, tmp_path):
    exe = str(tmp_path / "clearance_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "clearance_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/clearance_caller.cpp through include/hpsdf_octree.hpp: the structs and the cells it prints are the Python binding's."""
    A, B = _built(H, ctx, "union3_1e-5"), _built(H, ctx, "sphere075_1e-6")
    pose = general_pose(H, BUILT_POSE_T)
    exe = build_clearance_caller(H, tmp_path)
    (tmp_path / "a.bin").write_bytes(A)
    (tmp_path / "b.bin").write_bytes(B)
    (tmp_path / "pose.bin").write_bytes(pose.tobytes())
    r = subprocess.run([exe, str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "pose.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = parse_clearance_native(H, r.stdout)

    def same(tag, res):
        assert got[tag][0] == res.raw, tag
        if res.cells is not None:
            assert np.array_equal(got[tag][1], res.cells), tag

    same("a", H.clearance_block(A, A, None, 0.0, 6))
    assert len(got["a"][1]) == 0
    same("b", H.clearance_block(A, B, pose, 0.013, 6, 1e-3, 1 << 24, 64, cells=True))
    limited = H.clearance_block(A, B, pose, 0.0, 7, 0.0, 512, 256, cells=True)
    same("c", limited)
