"""Simplify without a device (include/hpsdf.h, "Simplify"): hpsdf_simplify_block against tests/simplify_reference.py -- the tables from
their integral, the rule replayed in long double, an independent L2 distance -- on hand-made blocks and on trees the CPU oracle built.
Every tolerance is a rounding bound derived in simplify_reference.py's docstring."""
import os
import re
import subprocess

import numpy as np
import pytest

import hiprec as HR
import simplify_reference as SR
from conftest import ROOT
from helpers import deep_chain_block, edge_points, oracle_field, query_points, synthetic_block
from hiprec import COUNT, INTERIOR, LD, U

RMS = (1e-4, 1e-3, 1e-2)
TREES = (("sphere", 1e-4), ("union3", 1e-5))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def trees(O):
    return {name: O.Tree.create(O.default_config(target), oracle_field(O, name), 1024).to_block() for name, target in TREES}


@pytest.fixture(scope="module")
def cases(H, trees):
    """(tree, rms) -> dict(source, result, stats, replay): computed once, shared, never modified."""
    out = {}
    for name, _ in TREES:
        for rms in RMS:
            result, stats = H.simplify_block(trees[name], rms)
            out[name, rms] = {"source": trees[name], "result": result, "stats": stats, "replay": SR.replay(trees[name], rms)}
    return out


# ------------------------------------------------------------------------------------------------------------ 1
def test_tables(H):
    T = H.simplify_transfer()
    want, zero = SR.transfer_tables()
    w64 = want.astype(np.float64)
    assert T.shape == (2, 13, 13)
    assert (T[zero] == 0.0).all() and (T[:, np.triu_indices(13, 1)[0], np.triu_indices(13, 1)[1]] == 0.0).all()
    off = np.abs(T.astype(LD) - want).astype(np.float64)
    assert (off[~zero] <= np.spacing(np.abs(w64[~zero]))).all(), (off[~zero] / np.spacing(np.abs(w64[~zero]))).max()
    assert not zero[:, np.arange(13), np.arange(13)].any()
    gram = sum(T[s] @ T[s].T for s in range(2))
    assert np.abs(gram - np.eye(13)).max() <= 30 * U * SR.SLACK


# ------------------------------------------------------------------------------------------------------------ 2
def _exact_merge_case(rng):
    degrees = [4, 4, 4, 1, 2, 4, 2, 1]       # parents of degree 1 and 2 have their children stored at degree 4, with zero tails
    return SR.exact_merge_block(rng, degrees, 4) + (degrees,)


def test_exact_merge(H):
    blk, parents, degrees = _exact_merge_case(np.random.default_rng(41))
    out, st = H.simplify_block(blk, 1e-9)
    res = HR.Block(out)
    assert len(res.degree) == 9 and st["nodes_out"] == 9 and st["merges"] == 8 and st["leaves_out"] == 8 and st["levels"] == 1
    rep = SR.replay(blk, 1e-9)
    assert rep["merged"] == set(range(1, 9)) and not rep["merge_doubt"]
    energy = 0.0
    for p in range(8):
        node = 1 + p
        # the merge keeps the children's stored degree, the truncation then drops the zero tails: back to the parent's degree
        assert res.degree[node] == degrees[p] == rep["degree"][node]
        got = res.coeffs[res.start[node]:res.start[node] + int(COUNT[degrees[p]])]
        want, bound = rep["rows"][node], rep["drows"][node]
        assert (np.abs(got.astype(LD) - want).astype(np.float64) <= bound).all()
        # and the replay's parent is the parent the children were made from, to the rounding of the children (u a row, through |T|^3)
        true = parents[p]
        # (a child's rows have at most the parent's norm: the bases are orthonormal and the child's cell lies inside the parent's)
        assert np.abs((want - true).astype(np.float64)).max() <= 8 * 13 ** 3 * U * float(np.sqrt((true * true).sum()))
        energy += float((true * true).sum())
    # e_step is the square of a rounding error: (K u)^2 of the energy, K the longest chain (simplify_reference.py, section 2)
    de = sum(float(rep["de"][1 + p]) for p in range(8))
    print("error_bound %.3g, derived bound %.3g, (150 u)^2 energy %.3g" % (st["error_bound"], de, (150 * U) ** 2 * energy))
    assert 0.0 <= st["error_bound"] <= de * SR.SLACK
    assert de <= (1000 * U) ** 2 * energy          # (the derived bound is itself of that order: the check above is not vacuous)
    # the shortcut sum |c_n|^2 - |parent|^2 cannot pass: its rounding alone is u times the energy
    short = 0.0
    src = HR.Block(blk)
    for p in range(8):
        kids = sum(float((src.coeffs[src.start[9 + 8 * p + n]:src.start[9 + 8 * p + n] + 35] ** 2).sum()) for n in range(8))
        got = res.coeffs[res.start[1 + p]:res.start[1 + p] + int(COUNT[degrees[p]])]
        short += abs(kids - float((got ** 2).sum()))
    assert short > de * SR.SLACK


# ------------------------------------------------------------------------------------------------------------ 3
def test_nothing_to_merge(H):
    rng = np.random.default_rng(43)
    for degrees in ([2] * 8, [0, 1, 2, 3, 4, 5, 6, 7], [12, 3, 3, 3, 3, 3, 3, 6]):
        blk = synthetic_block(rng, degrees, depth=2)
        out, st = H.simplify_block(blk, 1e-3)
        assert out == blk and st["merges"] == 0 and st["truncations"] == 0 and st["nodes_out"] == st["nodes_in"] == 17, degrees


# ------------------------------------------------------------------------------------------------------------ 4
def test_rms_zero_is_the_source(H, trees):
    for name, blk in trees.items():
        out, st = H.simplify_block(blk, 0.0)
        assert out == blk, name
        assert st["merges"] == st["truncations"] == st["levels"] == 0 and st["error_bound"] == 0.0 and st["coeffs_out"] == st["coeffs_in"]


# ------------------------------------------------------------------------------------------------------------ 5
def test_replay(cases):
    for (name, rms), c in cases.items():
        rep = c["replay"]
        src = rep["block"]
        pair, res = SR.result_leaves(c["source"], c["result"])
        got_degree = np.full(len(src.degree), -1, np.int64)
        got_degree[pair] = res.degree
        got_merged = {int(i) for i in np.nonzero((src.degree == INTERIOR) & (got_degree >= 0) & (got_degree != INTERIOR))[0]}
        # (merges below a merged node are not visible in the result; they are compared through stats["merges"])
        want_degree = rep["degree"]
        # a decision in doubt taints its cell and every cell above it
        doubt = set(rep["merge_doubt"]) | set(rep["trunc_doubt"])
        tainted = np.zeros(len(src.degree), bool)
        for i in doubt:
            tainted[i] = True
        for i in range(len(src.degree) - 1, -1, -1):       # (children come after their parent in a built tree's node array)
            if src.degree[i] == INTERIOR and rep["depth"][i] >= 0 and tainted[int(src.child[i]):int(src.child[i]) + 8].any():
                tainted[i] = True
        differ = np.nonzero(got_degree != want_degree)[0]
        excused = 0
        for i in differ:
            up, ok = int(i), False
            # the cell itself, or the surviving cell above it, must be tainted
            while True:
                if tainted[up]:
                    ok = True
                    break
                parents = np.nonzero((src.degree == INTERIOR) & (src.child <= up) & (up < src.child + 8))[0]
                if up == 0 or len(parents) == 0:
                    break
                up = int(parents[0])
            assert ok, (name, rms, int(i), int(got_degree[i]), int(want_degree[i]))
            excused += 1
        print(name, rms, "decisions %d, in doubt %d, differing nodes %d" % (rep["decisions"], len(doubt), len(differ)))
        assert len(doubt) == 0, "the long-double replay itself has a decision within rounding of its threshold: pick another rms"
        assert excused <= 0.01 * rep["decisions"]
        if len(differ) == 0:
            assert got_merged == {i for i in rep["merged"] if want_degree[i] >= 0}
            assert c["stats"]["merges"] == len(rep["merged"])
            for r in np.nonzero(res.degree != INTERIOR)[0]:
                s = int(pair[r])
                got = res.coeffs[res.start[r]:res.start[r] + int(COUNT[res.degree[r]])]
                assert (np.abs(got.astype(LD) - rep["rows"][s]).astype(np.float64) <= rep["drows"][s]).all(), (name, rms, s)


# ------------------------------------------------------------------------------------------------------------ 6
def test_guarantee(cases):
    for (name, rms), c in cases.items():
        st = c["stats"]
        total, per, energy = SR.l2_distance(c["source"], c["result"])
        res = HR.Block(c["result"])
        depth = SR.tree_depths(res)
        levels = int(SR.tree_depths(HR.Block(c["source"])).max())
        worst = 0.0
        for r, dist in per.items():
            vol = SR.volume(depth[r])
            allowed = float(rms) ** 2 * float(vol) * (1.0 + SR.guarantee_slack(energy[r], rms, vol, levels))
            worst = max(worst, float(dist) / (float(rms) ** 2 * float(vol)))
            assert float(dist) <= allowed, (name, rms, r, float(dist), allowed)
        e_total = float(sum(energy.values()))
        kg = 2 * levels * (SR.K_FWD + SR.K_BWD + SR.K_SUM) + 300
        allowed = st["error_bound"] + kg * U * (st["error_bound"] + np.sqrt(st["error_bound"] * e_total)) + (kg * U) ** 2 * e_total
        print(name, rms, "L2^2 %.6g <= error_bound %.6g; worst cell at %.4f of its budget; max_cell_rms %.6g" %
              (float(total), st["error_bound"], worst, st["max_cell_rms"]))
        assert float(total) <= allowed
        assert st["max_cell_rms"] <= rms


# ------------------------------------------------------------------------------------------------------------ 7
def test_a_readable_block(H, O, cases):
    rng = np.random.default_rng(47)
    for (name, rms), c in cases.items():
        out = c["result"]
        res = HR.Block(out)
        pts = np.concatenate([query_points(O, (-0.5,) * 3, (0.5,) * 3, 10000), res.from_unit(edge_points(rng))])
        want = O.Tree.from_block(out).query(pts)
        got = H.query_gradient_block(out, pts)[0]          # the product's host Query (it validates the block as hpsdf_tree_upload does)
        assert np.array_equal(_bits(got), _bits(want)), (name, rms)
        nn = len(res.degree)
        assert nn % 8 == 1 and nn == c["stats"]["nodes_out"]
        interior = np.nonzero(res.degree == INTERIOR)[0]
        assert ((res.child[interior].astype(np.int64) - 1) % 8 == 0).all()
        assert (res.child[res.degree != INTERIOR] == np.uint64(HR.LEAF)).all()
        # offsets increase along the depth-first walk (children 0 .. 7) without gaps and end at nCoeffs
        at, stack = 0, [0]
        while stack:
            i = stack.pop()
            if res.degree[i] == INTERIOR:
                stack.extend(range(int(res.child[i]) + 7, int(res.child[i]) - 1, -1))
            else:
                assert res.start[i] == at, (name, rms, i)
                at += int(COUNT[res.degree[i]])
        assert at == len(res.coeffs) == c["stats"]["coeffs_out"]


# ------------------------------------------------------------------------------------------------------------ 8
def test_flags(H, trees):
    for name, blk in trees.items():
        src = HR.Block(blk)
        merged, st = H.simplify_block(blk, 1e-3, truncate=False)
        pair, res = SR.result_leaves(blk, merged)
        assert st["truncations"] == 0 and st["merges"] > 0
        kept = (res.degree != INTERIOR) & (src.degree[pair] != INTERIOR)
        assert kept.any() and (res.degree[kept] == src.degree[pair][kept]).all()
        cut, st = H.simplify_block(blk, 1e-3, merge=False)
        nc = int(np.frombuffer(cut[:8], np.uint64)[0])
        res = HR.Block(cut)
        assert st["merges"] == 0 and st["truncations"] > 0 and st["nodes_out"] == st["nodes_in"] and nc < len(src.coeffs)
        assert np.array_equal(res.child, src.child) and np.array_equal(res.bmin, src.bmin) and np.array_equal(res.depth, src.depth)
        assert (res.degree <= src.degree).all() and (res.degree < src.degree).any()
        both, st = H.simplify_block(blk, 1e-3, flags=3)
        assert both == H.simplify_block(blk, 1e-3)[0]
        none, st = H.simplify_block(blk, 1e-3, flags=0)
        assert none == blk


# ------------------------------------------------------------------------------------------------------------ 9
def test_arguments(H, trees):
    import ctypes as C
    blk = trees["sphere"]
    L = H.lib()

    def raw(block, rms, flags, null_out=False):
        out, size, st = C.c_void_p(0xDEAD), C.c_size_t(0xBEEF), H.SimplifyStats()
        st.merges = 77
        rc = L.hpsdf_simplify_block(block, len(block), rms, flags, None if null_out else C.byref(out), C.byref(size), C.byref(st))
        return rc, out.value, size.value, st.merges

    for rms in (-1.0, float("nan"), float("inf"), -0.0 - 1e-300):
        assert raw(blk, rms, 3) == (H.ERR_INVALID_ARGUMENT, 0xDEAD, 0xBEEF, 77), rms
    for flags in (4, 7, 1 << 31):
        assert raw(blk, 1e-3, flags) == (H.ERR_INVALID_ARGUMENT, 0xDEAD, 0xBEEF, 77), flags
    assert raw(blk, 1e-3, 3, null_out=True)[0] == H.ERR_INVALID_ARGUMENT
    assert raw(blk[:-8], 1e-3, 3) == (H.ERR_BAD_BLOCK, 0xDEAD, 0xBEEF, 77)
    bad = bytearray(synthetic_block(np.random.default_rng(1), [2] * 8, depth=2))
    nc = int(np.frombuffer(bytes(bad[:8]), np.uint64)[0])
    bad[16 + 8 * nc + 56 + 8:16 + 8 * nc + 56 + 12] = np.array([-0.4], np.float32).tobytes()     # child 1's box is no octant
    assert raw(bytes(bad), 1e-3, 3) == (H.ERR_UNSUPPORTED, 0xDEAD, 0xBEEF, 77)
    with pytest.raises(H.HpsdfError) as ei:
        H.simplify_block(blk, -1.0)
    assert ei.value.status == H.ERR_INVALID_ARGUMENT
    # a NaN coefficient: accepted, and the cells it reaches stay as they are
    good, parents, degrees = _exact_merge_case(np.random.default_rng(41))
    src = HR.Block(good)
    poisoned = bytearray(good)
    at = 8 + 8 * int(src.start[9 + 5]) + 8      # row 1 of leaf 5 under child 0 (a parent of degree 4: no leaf under it has a zero tail)
    poisoned[at:at + 8] = np.array([np.nan]).tobytes()
    out, st = H.simplify_block(bytes(poisoned), 1e-9)
    res = HR.Block(out)
    assert st["merges"] == 7 and len(res.degree) == 17 and res.degree[1] == INTERIOR and res.child[1] == 9
    assert np.isfinite(st["error_bound"]) and np.isnan(res.coeffs).sum() == 1
    assert (res.degree[9:17] == 4).all() and (res.degree[2:9] == np.array(degrees[1:])).all()


def test_new_symbols_are_declared_bound_and_exported(H):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_simplify", "hpsdf_simplify_block", "hpsdf_simplify_transfer"}
    assert new <= declared and declared == set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    m = re.search(r"enum \{ HPSDF_SIMPLIFY_MERGE = (\d), HPSDF_SIMPLIFY_TRUNCATE = (\d) \}", hdr)
    assert tuple(int(x) for x in m.groups()) == (H.SIMPLIFY_MERGE, H.SIMPLIFY_TRUNCATE) == (SR.MERGE, SR.TRUNCATE) == (1, 2)
    assert C.sizeof(H.SimplifyStats) == 88
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == 4 == H.ABI_VERSION
    assert hasattr(H.Octree, "Simplify") and "Simplify(" in open(os.path.join(ROOT, "include", "hpsdf_octree.hpp")).read()


# ------------------------------------------------------------------------------------------------------------ 10
def build_caller(H, tmp_path):
    exe = str(tmp_path / "simplify_caller")
    libdir = os.path.dirname(H.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-comment", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "simplify_caller.cpp"), "-o", exe, "-L", libdir, "-lhpsdf", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def run_caller(exe, tmp_path, blk, rms, flags, where):
    (tmp_path / "in.bin").write_bytes(blk)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), repr(float(rms)), str(flags), where], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = dict((ln.split()[0], ln.split()[1:]) for ln in r.stdout.splitlines())
    assert lines["U"] == ["1"]
    f = lines["S"]
    keys = ("nodes_in", "coeffs_in", "leaves_in", "nodes_out", "coeffs_out", "leaves_out", "merges", "truncations", "levels")
    stats = {k: int(v) for k, v in zip(keys, f[:9])}
    stats["error_bound"], stats["max_cell_rms"] = (float(np.array([int(x, 16)], np.uint64).view(np.float64)[0]) for x in f[9:11])
    return (tmp_path / "out.bin").read_bytes(), stats


def test_cxx_caller(H, trees, tmp_path):
    """tests/native/simplify_caller.cpp through include/hpsdf_octree.hpp, host path: the Python binding's bytes and stats."""
    exe = build_caller(H, tmp_path)
    for rms, flags in ((1e-3, 3), (1e-2, 1)):
        got, stats = run_caller(exe, tmp_path, trees["union3"], rms, flags, "host")
        want, st = H.simplify_block(trees["union3"], rms, flags=flags)
        assert got == want and stats == st
