"""IntegratePair without a device: hpsdf_integrate_pair_block (the statements of the kernels on the calling thread).  Identities with
Integrate byte for byte; decided cells sound against Query of both trees with no tolerance; the image box against exact rational
arithmetic; the classification against the replay of tests/integrate_pair_reference.py; exact consistency between the operations and
nesting in the depth; the lens of two spheres against its analytic volume; limits, statuses, argument checks and symbols; a sanitizer
run of the host code as a stand-alone program."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hiprec as R
import integrate_pair_reference as PR
import integrate_reference as IR
from conftest import ROOT
from helpers import synthetic_block
from test_integrate_cpu import assert_native_equals, assert_tiling, parse_native, points_in_cells, synthetic_iso
from test_query_bounds_cpu import _golden_block
from test_surface_sparse_cpu import SPHERE_C, SPHERE_R, blocks  # noqa: F401  (blocks: the module's fixture of built trees)

CSRC = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "csrc")
OPS = (PR.INTERSECTION, PR.UNION, PR.DIFFERENCE)


def constant_block(value, root=1.0):
    """8 leaves of degree 0, every coefficient `value`, on the root [-root, root]^3"""
    blk = bytearray(synthetic_block(np.random.default_rng(3), [0] * 8, 1, (-root,) * 3, (root,) * 3))
    nc = int(np.frombuffer(bytes(blk[:8]), np.uint64)[0])
    assert nc == 8
    blk[8:8 + 8 * nc] = np.full(nc, value).tobytes()
    return bytes(blk)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def general_pose(H, t=(0.31, 0.17, -0.12)):
    """a rotation, a shear and a translation; with t it leaves B's root cutting through A's (both [-0.5, 0.5]^3)"""
    shear = np.array([[1.0, 0.15, 0.0], [0.0, 1.0, -0.1], [0.05, 0.0, 1.0]])
    return H.pose(rotation((0.3, -0.5, 0.8), 0.6) @ shear, t)


def images(pose, x):
    """y = M x + t for the rows of x, in the header's association"""
    P = np.asarray(pose).reshape(3, 4)
    return np.stack([((P[j, 0] * x[:, 0] + P[j, 1] * x[:, 1]) + P[j, 2] * x[:, 2]) + P[j, 3] for j in range(3)], 1)


# ------------------------------------------------------------------------------------------------------------ 1. identities
@pytest.mark.parametrize("name", ["union3_1e-5", "sphere_1e-6"])
def test_identities_with_integrate_byte_for_byte(H, blocks, name):
    A = blocks[name][0]
    want = H.integrate_block(A, 0.0, 6, 2, cells=True)
    inside, outside = constant_block(-1.0), constant_block(1.0)

    def same(res, what):
        assert res.raw == want.raw and res.cells.tobytes() == want.cells.tobytes(), what

    same(H.integrate_pair_block(A, inside, PR.INTERSECTION, None, depth=6, cells=True), "A n everything")
    same(H.integrate_pair_block(A, outside, PR.UNION, None, depth=6, cells=True), "A u nothing")
    same(H.integrate_pair_block(A, outside, PR.DIFFERENCE, None, depth=6, cells=True), "A minus nothing")
    assert H.integrate_pair_block(A, inside, PR.INTERSECTION, depth=6).raw == want.raw     # without the cells: the struct alone
    away = H.pose(None, (5.0, 0.0, 0.0))                                                   # A's root wholly outside B's root
    for B in (inside, outside):
        res = H.integrate_pair_block(A, B, PR.INTERSECTION, away, depth=6, cells=True)
        assert res.volume_hi == 0.0 and res.levels == 0 and (res.cells["cls"] == 1).all() and res.disjoint and not res.overlapping
        assert_tiling(res, "away")
        same(H.integrate_pair_block(A, B, PR.UNION, away, depth=6, cells=True), "A u (B out of reach)")
        same(H.integrate_pair_block(A, B, PR.DIFFERENCE, away, depth=6, cells=True), "A minus (B out of reach)")
    everything = H.integrate_pair_block(A, inside, PR.UNION, None, depth=6, cells=True)     # B decides every cell at level 0
    assert everything.unit_volume_lo == 1.0 and everything.levels == 0


# ------------------------------------------------------------------------------------------------------------ 2. soundness
def assert_pair_sound(H, A, B, res, op, pose, iso_a, iso_b, rng, what):
    c = res.cells
    counts = []
    for cls in (2, 1):
        pick = np.nonzero(c["cls"] == cls)[0]
        if len(pick) > 20000:
            pick = np.sort(rng.choice(pick, 20000, replace=False))
        x = points_in_cells(H, A, c[pick], rng).reshape(-1, 3)
        qa = H.query_gradient_block(A, x)[0]                                    # its value is Query's, bit for bit
        assert int((qa > 1e300).sum()) == 0, (what, "points that fail Query's containment test")
        qb = H.query_gradient_block(B, images(pose, x))[0]                      # DBL_MAX outside B's root: not in SB
        holds = PR.predicate(op, qa < iso_a, qb < iso_b)
        bad = np.nonzero(~holds if cls == 2 else holds)[0]
        assert len(bad) == 0, (what, cls, len(bad), c[pick][bad[:3] // 9].tolist(), qa[bad[:3]].tolist(), qb[bad[:3]].tolist())
        counts.append(len(pick))
    return counts


@pytest.mark.parametrize("pair", [("union3_1e-5", "sphere_1e-6"), ("sphere_1e-6", "sphere_1e-6")])
def test_decided_cells_are_sound_against_query_of_both_trees(H, blocks, pair):
    A, B = blocks[pair[0]][0], blocks[pair[1]][0]
    pose = general_pose(H)
    rng = np.random.default_rng(1201)
    for op in OPS:
        for iso_a, iso_b in ((0.0, 0.0), (0.013, -0.02)):
            res = H.integrate_pair_block(A, B, op, pose, iso_a, iso_b, 7, 2, cells=True)
            assert res.status == H.INTEGRATE_OK
            assert_tiling(res, (pair, op))
            n_in, n_out = assert_pair_sound(H, A, B, res, op, pose, iso_a, iso_b, rng, (pair, op, iso_a))
            assert n_in > 100 and n_out > 100
            print("%s op %d iso %g: %d inside and %d outside cells sampled, 9 points each" % (pair, op, iso_a, n_in, n_out))
    # B's root cuts through A's root: some of A's cells have images partly outside B's root (the clamp and `partial`), some wholly
    corners = np.array([[sx, sy, sz] for sx in (-0.5, 0.5) for sy in (-0.5, 0.5) for sz in (-0.5, 0.5)])
    y = images(pose, corners)
    out = (np.abs(y) > 0.5).any(1)
    assert out.any() and not out.all()


# ------------------------------------------------------------------------------------------------------------ 3. the box
def _random_box_cases(n):
    rng = np.random.default_rng(1213)
    for _ in range(n):
        rmin = (rng.uniform(-3, 3, 3) * 10.0 ** rng.uniform(-2, 2, 3)).astype(np.float32)
        rmax = rmin + (10.0 ** rng.uniform(-2, 2, 3)).astype(np.float32)
        centre, size = PR.root_map(rmin, rmax)
        depth = int(rng.integers(1, 16))
        ijk = [int(v) for v in rng.integers(0, 1 << depth, 3)]
        pose = [float(v) for v in rng.uniform(-1, 1, 12) * 10.0 ** rng.uniform(-3, 3, 12)]
        yield centre, size, pose, depth, ijk


def _box_holds(centre, size, pose, depth, ijk, slack):
    a, b = PR.image_box(centre, size, pose, depth, ijk, slack)
    fa, fb = [Fraction(v) for v in a], [Fraction(v) for v in b]
    for y in PR.exact_corner_images(centre, size, pose, depth, ijk):           # the image of a box is the hull of its corners' images
        if not all(fa[j] <= y[j] <= fb[j] for j in range(3)):
            return False
    for y in PR.sample_images(centre, size, pose, depth, ijk):
        if not all(a[j] <= y[j] <= b[j] for j in range(3)):
            return False
    return True


def test_the_image_box_contains_the_exact_image_and_every_sample(H):
    bare = 0
    for case in _random_box_cases(2000):
        assert _box_holds(*case, True), case
        bare += not _box_holds(*case, False)
    print("without delta %d of 2000 boxes lose a corner or a sample" % bare)
    assert bare >= 1                                                           # the test can see the slack
    # PMAX, PMIN and their outer neighbours cast as the header says
    half = np.float32(0.5)
    assert PR.PMAX == 0.5 + 2.0 ** -25 and np.float32(PR.PMAX) == half and np.float32(np.nextafter(PR.PMAX, 1.0)) > half
    assert np.float32(PR.PMIN) == -half and np.float32(np.nextafter(PR.PMIN, -1.0)) < -half
    assert PR.SLACK == 2.0 ** -48


# ------------------------------------------------------------------------------------------------------------ 4. the replay
def test_the_classification_follows_the_headers_rule(H):
    rng = np.random.default_rng(1217)
    A = synthetic_block(rng, [3, 5, 2, 7, 1, 4, 6, 0], 2, (-0.4, -0.3, -0.6), (0.5, 0.9, 0.1))
    B = synthetic_block(rng, [2, 0, 4, 1, 3, 9, 2, 5], 2, (-0.7, -0.5, -0.4), (0.6, 0.8, 0.9))
    iso_a, iso_b = synthetic_iso(H, A), synthetic_iso(H, B)
    pose = general_pose(H, (0.12, 0.2, 0.25))
    total = {"checked": 0, "ambiguous": 0, "walks": 0}
    for op in OPS:
        for max_leaves in (256, 3):
            res = H.integrate_pair_block(A, B, op, pose, iso_a, iso_b, 4, 1, max_leaves=max_leaves, cells=True)
            assert res.status == H.INTEGRATE_OK
            got = PR.replay_lists(A, B, res, op, pose, iso_a, iso_b, 4, max_leaves)
            print("op %d max_leaves %d:" % (op, max_leaves), got)
            assert got["wrong_class"] == 0, got
            assert got["lengths"] == IR.list_lengths(A, res) and len(got["lengths"]) == res.levels + 1
            assert res.evaluations == sum(got["lengths"]) + res.cells_undecided
            for k in total:
                total[k] += got[k]
    assert total["ambiguous"] <= 0.001 * total["checked"] and total["checked"] > 3000 and total["walks"] > 1000, total


# ------------------------------------------------------------------------------------------------------------ 5. exact consistency
@pytest.mark.parametrize("pair", [("union3_1e-5", "sphere_1e-6"), ("sphere_1e-6", "union3_1e-5")])
def test_the_enclosures_are_consistent_and_nest(H, blocks, pair):
    A, B = blocks[pair[0]][0], blocks[pair[1]][0]
    pose = general_pose(H)
    before = None
    for D in (3, 5, 7):
        one = H.integrate_block(A, 0.0, D, 1)
        r = {op: H.integrate_pair_block(A, B, op, pose, depth=D, samples=1) for op in OPS}
        lo = {op: Fraction(r[op].unit_volume_lo) for op in OPS}                # volumes are exact rationals: plain comparisons
        hi = {op: Fraction(r[op].unit_volume_hi) for op in OPS}
        assert lo[PR.INTERSECTION] + lo[PR.DIFFERENCE] <= Fraction(one.unit_volume_hi)
        assert hi[PR.INTERSECTION] + hi[PR.DIFFERENCE] >= Fraction(one.unit_volume_lo)
        assert lo[PR.UNION] >= Fraction(one.unit_volume_lo)
        for op in OPS:
            assert lo[op] <= Fraction(r[op].unit_volume) <= hi[op]
            if before:
                assert before[0][op] <= lo[op] and hi[op] <= before[1][op], (D, op)
        before = (lo, hi)
        print(pair, D, {op: (float(lo[op]), float(hi[op])) for op in OPS})


# ------------------------------------------------------------------------------------------------------------ 6. the lens
def test_the_lens_of_two_spheres(H, blocks):
    S = blocks["sphere_1e-6"][0]
    c, Rad = np.array(SPHERE_C), SPHERE_R
    t = np.array((0.25, 0.1, -0.05))
    d = float(np.linalg.norm(t))
    V = math.pi * (4 * Rad + d) * (2 * Rad - d) ** 2 / 12
    # eps: the fitted field against the analytic one, over points within 0.05 of the surface
    rng = np.random.default_rng(1223)
    u = rng.standard_normal((40000, 3))
    x = c + u / np.linalg.norm(u, axis=1)[:, None] * (Rad + rng.uniform(-0.05, 0.05, (40000, 1)))
    x = x[(np.abs(x) < 0.5).all(1)]
    assert len(x) >= 20000
    eps = float(np.abs(H.query_gradient_block(S, x)[0] - (np.linalg.norm(x - c, axis=1) - Rad)).max())
    m = 2 * 4 * math.pi * Rad ** 2 * eps
    for D in (5, 7):
        res = H.integrate_pair_block(S, S, PR.INTERSECTION, H.pose(None, t), depth=D, samples=4)
        print("lens D=%d: V = %.9f in [%.9f, %.9f], estimate %.9f, eps %.3g, margin %.3g" % (D, V, res.volume_lo, res.volume_hi, res.volume, eps, m))
        assert res.status == H.INTEGRATE_OK and res.overlapping and not res.disjoint
        assert res.volume_lo - m <= V <= res.volume_hi + m
        assert res.volume_lo <= res.volume <= res.volume_hi
        # the centroid lies on the line of centres: the estimate's first moment about that line differs from the true solid's -- zero
        # for two analytic spheres -- by at most the undecided volume (and the margin) times the largest distance from the centre
        U = res.volume_hi - res.volume_lo
        off = res.centroid - c
        off = off - (off @ t) / (t @ t) * t
        assert np.linalg.norm(off) * res.volume <= (U + m) * (Rad + math.sqrt(3) * 2.0 ** -D), (off, U)
        mid = c - 0.5 * t                                                       # the lens is symmetric about the midpoint of the centres
        assert abs((res.centroid - mid) @ t) / d * res.volume <= (U + m) * (Rad + math.sqrt(3) * 2.0 ** -D)


# ------------------------------------------------------------------------------------------------------------ 7. degradation
def test_limits_degrade_and_non_finite_coefficients_end_the_call(H, blocks):
    A, B = blocks["union3_1e-5"][0], blocks["sphere_1e-6"][0]
    pose = general_pose(H)
    rng = np.random.default_rng(1229)
    free = H.integrate_pair_block(A, B, PR.INTERSECTION, pose, depth=6, cells=True)
    one = H.integrate_pair_block(A, B, PR.INTERSECTION, pose, depth=6, max_leaves=1, cells=True)
    assert one.status == H.INTEGRATE_OK
    assert_tiling(one, "max_leaves 1")
    assert_pair_sound(H, A, B, one, PR.INTERSECTION, pose, 0.0, 0.0, rng, "max_leaves 1")
    assert one.unit_volume_lo <= free.unit_volume_lo and one.unit_volume_hi >= free.unit_volume_hi
    assert one.unit_volume_hi - one.unit_volume_lo > free.unit_volume_hi - free.unit_volume_lo
    lengths = IR.list_lengths(A, free)
    limited = H.integrate_pair_block(A, B, PR.INTERSECTION, pose, depth=6, max_cells=lengths[2] - 1, cells=True)
    assert limited.status == H.INTEGRATE_CELL_LIMIT and limited.levels == 1
    assert_tiling(limited, "limited")
    assert_pair_sound(H, A, B, limited, PR.INTERSECTION, pose, 0.0, 0.0, rng, "limited")
    assert limited.unit_volume_lo <= free.unit_volume_lo and limited.unit_volume_hi >= free.unit_volume_hi
    # a non-finite coefficient in B, and in A
    good = synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)
    Bk = R.Block(good)
    leaf = int(Bk.descend(np.array([[0.25, 0.25, 0.25]]))[0])
    iso = synthetic_iso(H, good)
    for bad in (np.inf, np.nan):
        raw = bytearray(good)
        at = 8 + 8 * int(Bk.start[leaf])
        raw[at:at + 8] = np.array([bad]).tobytes()
        for a_blk, b_blk in ((good, bytes(raw)), (bytes(raw), good)):
            for op in OPS:
                res = H.integrate_pair_block(a_blk, b_blk, op, None, iso, iso, 4, 2, cells=True)
                assert res.status == H.INTEGRATE_NOT_FINITE, (bad, op)
                assert (res.unit_volume_lo, res.unit_volume_hi, res.volume_lo, res.volume_hi) == (0.0, 1.0, 0.0, 1.0)
                assert np.isnan(res.unit_volume) and np.isnan(res.volume) and np.isnan(res.m1).all() and np.isnan(res.m2).all()
                assert (res.cells_inside, res.cells_outside, res.cells_undecided) == (0, 0, 0) and len(res.cells) == 0
                assert not res.disjoint and not res.overlapping
    assert H.integrate_pair_block(good, good, PR.UNION, None, iso, iso, 4, 2).status == H.INTEGRATE_OK


# ------------------------------------------------------------------------------------------------------------ 8. arguments, symbols
def test_argument_checks(H):
    blk = synthetic_block(np.random.default_rng(1231), [2, 1, 0, 2, 2, 1, 2, 0], 1)
    buf = bytes(blk)
    L = H.lib()
    st = H.hpsdf_integral()
    C.memset(C.byref(st), 7, C.sizeof(st))
    seven = bytes(st)
    ptr, count = C.c_void_p(77), C.c_uint64(77)
    identity = H.pose()

    def call(op=0, pose=identity, iso_a=0.0, iso_b=0.0, depth=4, samples=2, max_cells=4096, max_leaves=256, out=st, cells=True, raw_a=buf,
             raw_b=buf, count_too=True):
        return L.hpsdf_integrate_pair_block(raw_a, len(raw_a), raw_b, len(raw_b), op, pose.ctypes.data_as(C.c_void_p) if pose is not None else None,
                                            iso_a, iso_b, depth, samples, max_cells, max_leaves, C.byref(out) if out is not None else None,
                                            C.byref(ptr) if cells else None, C.byref(count) if cells and count_too else None)

    untouched = lambda: bytes(st) == seven and ptr.value == 77 and count.value == 77
    refused = lambda **kw: call(**kw) == H.ERR_INVALID_ARGUMENT and untouched()
    for v in (np.inf, -np.inf, np.nan):
        assert refused(iso_a=v) and refused(iso_b=v) and b"iso" in L.hpsdf_last_error()
        for k in (0, 5, 11):
            P = identity.copy()
            P[k] = v
            assert refused(pose=P) and b"pose" in L.hpsdf_last_error()
    assert refused(op=3) and refused(op=0xFFFFFFFF) and b"op" in L.hpsdf_last_error()
    assert refused(depth=16) and refused(samples=3) and refused(max_cells=7) and refused(max_cells=(1 << 28) + 1)
    assert refused(max_leaves=0) and refused(max_leaves=65536) and b"max_leaves" in L.hpsdf_last_error()
    assert refused(pose=None) and refused(out=None) and refused(count_too=False)
    for cut in (buf[:-1], buf[:100], b""):
        assert call(raw_a=cut) == H.ERR_BAD_BLOCK and untouched()
        assert call(raw_b=cut) == H.ERR_BAD_BLOCK and untouched()
    assert call(op=2, depth=15, samples=4, max_cells=1 << 28, max_leaves=65535) == H.OK and not untouched()   # the limits pass
    assert count.value > 0 and ptr.value
    L._libc.free(ptr)
    assert call(depth=0, samples=1, max_cells=8, max_leaves=1, cells=False) == H.OK
    with pytest.raises(H.HpsdfError) as ei:
        H.integrate_pair_block(blk, blk, 3)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT


def test_new_symbols_are_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_integrate_pair_device", "hpsdf_integrate_pair_host", "hpsdf_integrate_pair_block"}
    assert new <= declared and declared == set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    m = re.search(r"enum \{ HPSDF_PAIR_INTERSECTION = (\d), HPSDF_PAIR_UNION = (\d), HPSDF_PAIR_DIFFERENCE = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.PAIR_INTERSECTION, H.PAIR_UNION, H.PAIR_DIFFERENCE) == OPS == (0, 1, 2)
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == 4 == H.ABI_VERSION == H.lib().hpsdf_abi_version()
    assert C.sizeof(H.hpsdf_integral) == 24 * 8 + 4 * 8 + 2 * 4
    assert callable(H.DeviceTree.integrate_pair) and callable(H.Octree.IntegratePair) and callable(H.integrate_pair_block)
    assert np.array_equal(H.pose(), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) and np.array_equal(H.pose(None), H.pose())
    assert np.array_equal(H.pose(np.arange(9.0).reshape(3, 3), (9, 10, 11)), [0, 1, 2, 9, 3, 4, 5, 10, 6, 7, 8, 11])
    assert isinstance(H.PairIntegral.disjoint, property) and isinstance(H.PairIntegral.overlapping, property)
    cxx = open(os.path.join(ROOT, "include", "hpsdf_octree.hpp")).read()
    assert "IntegratePair(const Octree& other_" in cxx


# ------------------------------------------------------------------------------------------------------------ 9. a sanitizer run
PAIR_MAIN_CASES = (("a", 0, 0, 1, 8, 256), ("b", 0, 6, 2, 1 << 24, 256), ("c", 1, 5, 4, 1 << 24, 2), ("d", 2, 7, 2, 4096, 256))


def pair_main_pose(H):
    return general_pose(H, (0.2, -0.1, 0.15))


def test_block_entry_is_clean_under_asan_ubsan(H, O, tmp_path, golden, blocks):
    """tests/native/integrate_pair_block_main.cpp: a stand-alone program (its own main, no library) that calls hpsdf_integrate_pair_block
    on two blocks, built with the host sources under AddressSanitizer and UBSan and run as a program.  What it prints -- the struct and
    the cells, as bits -- is the library's."""
    exe = str(tmp_path / "integrate_pair_block_main")
    srcs = [os.path.join(ROOT, "tests", "native", "integrate_pair_block_main.cpp")] + \
        [os.path.join(CSRC, f) for f in ("integrate_pair_host.cpp", "host_query.cpp", "tables.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include")] + srcs + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    A, B = _golden_block(O, golden), blocks["union3_1e-5"][0]
    pose = pair_main_pose(H)
    (tmp_path / "a.bin").write_bytes(A)
    (tmp_path / "b.bin").write_bytes(B)
    (tmp_path / "pose.bin").write_bytes(pose.tobytes())
    r = subprocess.run([exe, str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "pose.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    got = parse_native(r.stdout)
    for tag, op, depth, samples, max_cells, max_leaves in PAIR_MAIN_CASES:
        res = H.integrate_pair_block(A, B, op, pose, 0.0, 0.013, depth, samples, max_cells, max_leaves, cells=True)
        assert_native_equals(got[tag], res, tag)
    assert {int(got[t][0][0]) for t in got} == {H.INTEGRATE_OK, H.INTEGRATE_CELL_LIMIT}
