"""ClearanceBatch on the GPU: the kernels (clearance_batch.hip) and the _host entry against the device-free entry byte for byte over all
n structs (which tests/test_clearance_batch_cpu.py shows equal to the single call) -- runs of 8 cells sharing a wave, runs crossing a
workgroup boundary, wave-uniform runs, runs of several workgroups; poses that stop at different levels with different statuses in one
call; a constant B whose candidates all tie; independence of order, company and budget; a non-finite B for one pose only; `decide`;
n = 0 and 1; the argument checks; a C++ caller of the drop-in."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import clearance_reference as CR
from conftest import ROOT
from helpers import synthetic_block
from test_clearance_batch_cpu import SIZE, parse_batch_native
from test_gpu_integrate_pair import BUILT_POSE_T, DEGREES
from test_gpu_query_gradient import _built
from test_integrate_cpu import synthetic_iso
from test_integrate_pair_cpu import constant_block, general_pose

_blocks = {}


def built(H, ctx, name):
    if name not in _blocks:
        _blocks[name] = _built(H, ctx, name)
    return _blocks[name]


def check_batch(H, A, B, poses, args, what, trees, decide=None, max_total_cells=1 << 24, host=True):
    """device and host entries against the block entry -> the block entry's result"""
    want = H.clearance_batch_block(A, B, poses, *args, decide=decide)
    tA, tB = trees
    got = tA.clearance_batch(tB, poses, *args, decide=decide, max_total_cells=max_total_cells)
    differ = [i for i in range(len(want)) if got.raw[i * SIZE:(i + 1) * SIZE] != want.raw[i * SIZE:(i + 1) * SIZE]]
    assert not differ, (what, "device", differ, [(got[i], want[i]) for i in differ[:3]])
    if host:
        assert tA.clearance_batch(tB, poses, *args, decide=decide, host=True).raw == want.raw, (what, "host")
    return want


def some_poses(H, n, seed, spread=0.15):
    rng = np.random.default_rng(seed)
    return np.stack([general_pose(H, tuple(rng.uniform(-spread, spread, 3))) for _ in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["8", "8 then 64", "15", "4096"])
def test_segment_shapes(H, ctx, case):
    """Runs of 8 cells (eight poses in a wave; 33 poses: 264 cells, a run across the workgroup boundary), of 64 cells (list 1 of the
    8-leaf tree when every cell splits: 4 poses are wave-uniform runs in one workgroup, 5 poses 320 cells), of 15 cells (runs that start
    anywhere in a wave) and of 4096 cells (every pose spans several workgroups).  The lengths are asserted with the replay."""
    rng = np.random.default_rng(1801)
    mid = synthetic_block(rng, DEGREES[5], 2)                                    # list 0 has 15 cells
    small = synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)                    # list 0 has 8 cells
    other = synthetic_block(rng, DEGREES[3], 2)
    if case == "8":
        A, head, counts, D, iso_a = small, [8], (8, 33), 3, synthetic_iso(H, small)
    elif case == "8 then 64":
        A, head, counts, D, iso_a = small, [8, 64], (4, 5), 2, 1e300
    elif case == "15":
        A, head, counts, D, iso_a = mid, [15], (4, 5), 3, synthetic_iso(H, mid)
    else:
        A, head, counts, D, iso_a = built(H, ctx, "union3_1e-5"), [4096], (3,), 5, 1e-5   # list 0 is longer than a workgroup
    tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, other)
    for n in counts:
        poses = some_poses(H, n, 1811 + n)
        every = len(head) > 1                                                    # the runs of list 1 matter: replay every pose
        lengths = [CR.replay(H, A, other, p, iso_a, D)["lengths"] for p in (poses if every else poses[:1])]
        assert all(l[:len(head)] == head for l in lengths), lengths
        want = check_batch(H, A, other, poses, (iso_a, D, 0.0, 1 << 13, 256), ("shape", head, n), (tA, tB))
        assert int(want.cells_visited[0]) == sum(lengths[0]) and want.cells_visited.min() >= head[0]
    tA.close(), tB.close()


def mixed_poses(H):
    away = H.pose(None, (-2.0, -2.0, -2.0))                                      # A's image outside B's root: EMPTY
    return np.stack([general_pose(H, BUILT_POSE_T), H.pose(None, (3.0, 3.0, 3.0)), away, H.pose(), general_pose(H, BUILT_POSE_T)])


@pytest.mark.gpu
def test_poses_that_stop_at_different_levels_and_statuses_in_one_call(H, ctx):
    A, B = built(H, ctx, "union3_1e-5"), built(H, ctx, "sphere075_1e-6")
    trees = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    poses = mixed_poses(H)
    statuses, levels = set(), set()
    for tol, max_cells in ((0.0, 1 << 24), (0.05, 1 << 24), (0.0, 64)):
        want = check_batch(H, A, B, poses, (1e-5, 7, tol, max_cells, 256), ("mixed", tol, max_cells), trees)
        assert want.raw[:SIZE] == want.raw[4 * SIZE:5 * SIZE]                    # the duplicate
        statuses |= set(want.status.tolist())
        levels |= set(want.levels.tolist())
        print(tol, max_cells, want.status, want.levels, want.lo, want.hi)
    assert {H.CLEARANCE_DEPTH, H.CLEARANCE_CONVERGED, H.CLEARANCE_EMPTY, H.CLEARANCE_CELL_LIMIT} <= statuses, statuses
    assert len(levels) >= 3
    trees[0].close(), trees[1].close()


@pytest.mark.gpu
def test_decide_on_the_device(H, ctx):
    """the mixed poses with a threshold every pose decides on list 0 and one that lies inside one pose's enclosure, below another's and
    above a third's"""
    A, B = built(H, ctx, "union3_1e-5"), built(H, ctx, "sphere075_1e-6")
    trees = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    poses = mixed_poses(H)
    seen, levels = set(), set()
    for d in (1e-6, -0.6):
        want = check_batch(H, A, B, poses, (1e-5, 7, 0.0, 1 << 24, 256), ("decide", d), trees, decide=d, host=d > 0)
        seen |= set(want.status.tolist())
        levels |= set(want.levels[want.status == H.CLEARANCE_DECIDED].tolist())
        print(d, want.status, want.levels)
    assert H.CLEARANCE_DECIDED in seen and len(seen) >= 2 and len(levels) >= 2, (seen, levels)
    trees[0].close(), trees[1].close()


@pytest.mark.gpu
def test_every_candidate_of_every_pose_ties(H, ctx):
    """B constant: every candidate of a pose has the same vb, so its witness is the candidate of the smallest position IN ITS OWN RUN --
    the first cell of list 0 whose centre lies in A's solid, whatever the pose -- and not the smallest position of the combined list."""
    A = built(H, ctx, "union3_1e-5")
    const = constant_block(0.75)
    trees = H.DeviceTree(ctx, A), H.DeviceTree(ctx, const)
    poses = np.stack([H.pose(), H.pose(None, (0.05, -0.02, 0.01)), general_pose(H, (0.02, 0.01, -0.03))])
    want = check_batch(H, A, const, poses, (1e-5, 4, 0.0, 1 << 24, 256), ("ties",), trees)
    full = H.clearance_block(A, const, None, 1e300, 0, 1e300, cells=True)       # list 0 itself, in order
    boxes = H.cells_to_boxes(A, full.cells)
    centres = 0.5 * (boxes[:, :3] + boxes[:, 3:])
    first = int(np.nonzero(H.query_gradient_block(A, centres)[0] < 1e-5)[0][0])
    assert len(centres) > 256
    for i in range(len(poses)):
        assert np.isfinite(want.hi[i]) and np.array_equal(want.point[i], centres[first]), (i, want.point[i], centres[first])
    trees[0].close(), trees[1].close()


@pytest.mark.gpu
def test_independence_of_order_company_budget_and_other_calls(H, ctx):
    A, B = built(H, ctx, "union3_1e-5"), built(H, ctx, "sphere075_1e-6")
    tA, tB = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    poses = np.concatenate([mixed_poses(H), some_poses(H, 4, 1823, 0.5)])
    n = len(poses)
    args = (1e-5, 6, 0.0, 1 << 14, 256)
    want = check_batch(H, A, B, poses, args, ("all",), (tA, tB))
    row = lambda r, i: r.raw[i * SIZE:(i + 1) * SIZE]
    perm = np.random.default_rng(1831).permutation(n)
    got = tA.clearance_batch(tB, poses[perm], *args)
    assert all(row(got, k) == row(want, int(i)) for k, i in enumerate(perm))
    sub = [7, 2, 0]
    got = tA.clearance_batch(tB, poses[sub], *args)
    assert all(row(got, k) == row(want, i) for k, i in enumerate(sub))
    single = tA.clearance(tB, poses[0], *args)                                   # a plain call in between
    assert single.raw == row(want, 0)
    assert tA.clearance_batch(tB, poses, *args).raw == want.raw                  # a repeat call
    # a budget below n x len(list 0): the poses go in chunks
    list0 = int(CR.replay(H, A, B, poses[0], 1e-5, 0)["lengths"][0])
    for budget in (n * list0 - 1, 1 << 14):
        assert args[3] <= budget < n * list0
        assert tA.clearance_batch(tB, poses, *args, max_total_cells=budget).raw == want.raw, budget
    tA.close(), tB.close()


@pytest.mark.gpu
def test_a_budget_the_lists_outgrow_halves_the_chunks_and_starts_them_again(H, ctx):
    """The 8-leaf A: list 0 of all 33 poses fits max_total_cells = max_cells = 512, list 1 (64 cells a pose) does not, and list 2 of a
    few poses does not either: the chunks halve down to a few poses, some to one.  The bytes are the unconstrained call's."""
    rng = np.random.default_rng(1801)
    synthetic_block(rng, DEGREES[5], 2)
    A = synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)
    B = synthetic_block(rng, DEGREES[3], 2)
    poses = some_poses(H, 33, 1811 + 33)
    iso_a = synthetic_iso(H, A)
    lengths = [CR.replay(H, A, B, p, iso_a, 3, 0.0, 512)["lengths"] for p in poses[:4]]
    assert all(l[0] == 8 for l in lengths) and 33 * 8 <= 512 < 33 * min(l[1] for l in lengths) and max(max(l) for l in lengths) > 256, lengths
    trees = H.DeviceTree(ctx, A), H.DeviceTree(ctx, B)
    want = check_batch(H, A, B, poses, (iso_a, 3, 0.0, 512, 256), ("free",), trees, host=False)
    got = trees[0].clearance_batch(trees[1], poses, iso_a, 3, 0.0, 512, 256, max_total_cells=512)
    assert got.raw == want.raw
    trees[0].close(), trees[1].close()


@pytest.mark.gpu
def test_not_finite_for_one_pose_only(H, ctx):
    import hiprec as R
    good = synthetic_block(np.random.default_rng(1527), DEGREES[3], 2)
    Bk = R.Block(good)
    leaf = int(Bk.descend(np.array([[0.25, 0.25, 0.25]]))[0])
    raw = bytearray(good)
    at = 8 + 8 * int(Bk.start[leaf])
    raw[at:at + 8] = np.array([np.inf]).tobytes()
    bad = bytes(raw)
    iso = synthetic_iso(H, good)
    poses = np.stack([H.pose(), H.pose(0.2 * np.eye(3), (-0.3, -0.3, -0.3)), H.pose()])   # the second image stays clear of the leaf
    want = H.clearance_batch_block(good, bad, poses, iso, 4)
    assert want.status[0] == want.status[2] == H.CLEARANCE_NOT_FINITE and want.status[1] in (H.CLEARANCE_DEPTH, H.CLEARANCE_CONVERGED), want.status
    nf = want[0]
    assert nf.lo == -math.inf and nf.hi == math.inf and np.isnan(nf.point).all() and np.isnan(nf.value_a)
    assert (nf.cells_visited, nf.cells_outside_a, nf.cells_pruned, nf.cells_open) == (0, 0, 0, 0)
    tA, tB = H.DeviceTree(ctx, good), H.DeviceTree(ctx, bad)
    check_batch(H, good, bad, poses, (iso, 4, 0.0, 1 << 13, 256), ("not finite",), (tA, tB))
    tA.close(), tB.close()


@pytest.mark.gpu
def test_n_zero_n_one_and_argument_checks_leave_the_context_usable(H, ctx):
    blk = synthetic_block(np.random.default_rng(1561), [2, 1, 0, 2, 2, 1, 2, 0], 1)
    tree = H.DeviceTree(ctx, blk)
    pose = general_pose(H)
    assert len(tree.clearance_batch(tree, np.zeros((0, 12)), 0.1, 5)) == 0
    assert tree.clearance_batch(tree, [pose], 0.1, 5).raw == tree.clearance(tree, pose, 0.1, 5).raw
    L = H.lib()
    n = 3
    out = (H.hpsdf_clearance * n)()
    C.memset(out, 7, C.sizeof(out))
    seven = bytes(out)
    good = np.tile(H.pose(), (n, 1))
    bad_pose = good.copy()
    bad_pose[1, 3] = np.inf
    for fn in (L.hpsdf_clearance_batch_device, L.hpsdf_clearance_batch_host):
        def call(ta=tree.handle, tb=tree.handle, poses=good, count=n, decide=math.nan, max_cells=4096, max_total=4096, res=out, cx=ctx.handle, tol=0.0):
            return fn(cx, ta, tb, poses.ctypes.data_as(C.c_void_p) if poses is not None else None, count, 0.0, 4, tol, decide, max_cells, 256, max_total, res)
        refused = lambda **kw: call(**kw) == H.ERR_INVALID_ARGUMENT and bytes(out) == seven
        assert refused(poses=bad_pose) and refused(poses=None) and refused(decide=math.inf) and refused(tol=-1.0)
        assert refused(max_total=4095) and refused(max_total=(1 << 28) + 1) and refused(max_cells=7) and refused(count=(1 << 24) + 1)
        assert refused(res=None) and refused(ta=None) and refused(tb=None)
        assert call(cx=None) == H.ERR_NO_DEVICE and bytes(out) == seven
        assert call(count=0, poses=None, res=None) == H.OK and bytes(out) == seven
    poses = some_poses(H, 3, 1871)
    want = H.clearance_batch_block(blk, blk, poses, 0.1, 5)                      # the context and the tree still answer
    assert tree.clearance_batch(tree, poses, 0.1, 5).raw == want.raw
    assert tree.clearance_batch(tree, poses, 0.1, 5, host=True).raw == want.raw
    tree.close()


@pytest.mark.gpu
def test_cxx_caller(H, ctx, tmp_path):
    """tests/native/clearance_batch_caller.cpp through include/hpsdf_octree.hpp: the structs it prints are the Python binding's."""
    A, B = built(H, ctx, "union3_1e-5"), built(H, ctx, "sphere075_1e-6")
    poses = mixed_poses(H)
    exe = str(tmp_path / "clearance_batch_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "clearance_batch_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    (tmp_path / "a.bin").write_bytes(A)
    (tmp_path / "b.bin").write_bytes(B)
    (tmp_path / "poses.bin").write_bytes(poses.tobytes())
    r = subprocess.run([exe, str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "poses.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = parse_batch_native(r.stdout)
    assert got["a"] == H.clearance_batch_block(A, B, poses, 1e-5, 6).raw
    assert got["b"] == H.clearance_batch_block(A, B, poses, 1e-5, 6, 1e-3, 512, 64).raw
    assert got["c"] == H.clearance_batch_block(A, B, poses, 1e-5, 6, 0.0, 1 << 16, 256, decide=1e-6).raw
