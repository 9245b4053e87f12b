"""A replay of Clearance's rule (include/hpsdf.h, "Clearance"), written from the header's text in numpy and independent of the product's
clearance code.

  * The image box and the clamp are integrate_pair_reference.py's image_box and clamp (float64, the header's association).
  * A cell's class on A is integrate_reference.py's Replay.classify (long double); a cell it reports as ambiguous would make the replay
    undecidable and is counted (the tests assert that there is none).
  * blo has to be the product's double, or `blo <= best` could not be replayed: it is QueryBounds' answer (H.query_bounds_block, an
    entry with its own tests) on B with the unit root [-0.5, 0.5]^3 in its config -- that root's map is the identity, so the walk starts
    from the clamped range [pl, ph] itself, as unit_view does for bounds_reference.py.  check_walk > 0 also walks that many cells with
    bounds_reference.bounds_box on unit_view (long double) and asserts the double within bounds_reference's margin 2^-40 (S + e).
  * Query values (va, vb) are H.query_gradient_block's, which are Query's bit for bit.
replay(...) returns everything the rule defines: the list lengths, best after every level, the counters, lo, hi, the witness, the status
and the final cells in order.
"""
import numpy as np

import bounds_reference as BR
import integrate_pair_reference as PR
import integrate_reference as IR

CONVERGED, DEPTH, CELL_LIMIT, EMPTY, NOT_FINITE = 0, 1, 2, 3, 4
DBL_MAX = float(np.finfo(np.float64).max)
INF = float("inf")


def unit_root_block(blk):
    """the block with the root [-0.5, 0.5]^3 in its config (the last 24 bytes: root_min, root_max as float32)"""
    b = bytearray(blk)
    b[-24:] = np.array([-0.5] * 3 + [0.5] * 3, np.float32).tobytes()
    return bytes(b)


def cell_centre(centre, size, depth, ijk):
    """cx of the header's step 3"""
    s = 1.0 / float(1 << depth)
    return [centre[k] + ((-0.5 + float(ijk[k]) * s) + 0.5 * s) * size[k] for k in range(3)]


def replay(H, blk_a, blk_b, pose, iso_a, D, tol=0.0, max_cells=1 << 24, max_leaves=256, check_walk=0):
    pose = [float(v) for v in (H.pose() if pose is None else np.asarray(pose, np.float64).reshape(12))]
    rp = IR.Replay(blk_a)
    TB = BR.Tree(blk_b)
    VB = PR.unit_view(TB)
    unit_b = unit_root_block(blk_b)
    centre, size = PR.root_map(rp.B.root_min, rp.B.root_max)
    out = {"lengths": [], "best": [], "visited": 0, "outside_a": 0, "pruned": 0, "ambiguous": 0, "walk_checked": 0, "status": EMPTY,
           "lo": INF, "hi": INF, "point": None, "image": None, "value_a": None, "cells": [], "levels": 0}
    cur = [(int(n), int(rp.depth[n]), int(rp.ijk[n][0]), int(rp.ijk[n][1]), int(rp.ijk[n][2])) for n in rp.leaves]
    best, witness = INF, None
    finals = []                                                                # (cell, clsA, blo)
    level = 0
    while cur:
        n = len(cur)
        out["lengths"].append(n)
        out["visited"] += n
        out["levels"] = level
        arr = np.array(cur, np.int64)
        mask = (1 << level) - 1
        cls_a = np.zeros(n, np.int64)
        for node in np.unique(arr[:, 0]):
            sel = np.nonzero(arr[:, 0] == node)[0]
            c, amb = rp.classify(int(node), level, arr[sel, 2:5] & mask, iso_a)
            cls_a[sel] = c
            out["ambiguous"] += int(amb.sum())
        # step 1
        blo = np.full(n, INF)
        walked, boxes = [], []
        for i, (node, depth, ci, cj, ck) in enumerate(cur):
            if cls_a[i] == 1:
                continue
            a, b = PR.image_box(centre, size, pose, depth, (ci, cj, ck))
            reach, pl, ph, _ = PR.clamp(TB, a, b)
            if reach == 1:
                continue
            if reach == 3:
                blo[i] = -INF
                continue
            walked.append(i)
            boxes.append(list(pl) + list(ph))
        if walked:
            lo, _, status, _ = H.query_bounds_block(unit_b, np.array(boxes), 1, max_leaves)
            assert (status != BR.INVALID).all()
            if (status == BR.NOT_FINITE).any():
                out.update(status=NOT_FINITE, lo=-INF, hi=INF, cells=[])
                return out
            blo[walked] = lo
            for w in range(min(check_walk - out["walk_checked"], len(walked))):
                rlo, _, rstatus, _, S, e = BR.bounds_box(VB, np.array(boxes[w][:3]), np.array(boxes[w][3:]), 1, max_leaves)
                assert rstatus == status[w]
                if rstatus == BR.OK:
                    assert abs(BR.LD(lo[w]) - rlo) <= BR.LD(2.0 ** -40) * (BR.LD(S) + BR.LD(e)), (cur[walked[w]], lo[w], rlo)
                out["walk_checked"] += 1
        # step 2
        if walked:
            X = np.array([cell_centre(centre, size, cur[i][1], cur[i][2:5]) for i in walked])
            va = H.query_gradient_block(blk_a, X)[0]
            solid = np.nonzero(va < iso_a)[0]
            if len(solid):
                Y = np.array([PR.image(pose, [float(v) for v in X[s]]) for s in solid])
                vb = H.query_gradient_block(blk_b, Y)[0]
                cand = np.nonzero(vb < DBL_MAX)[0]
                if len(cand):
                    first = cand[np.argmin(vb[cand])]                          # argmin returns the first of equal values: the least pos
                    if vb[first] < best:
                        best = float(vb[first])
                        s = solid[first]
                        witness = (X[s].copy(), Y[first].copy(), float(va[s]))
        out["best"].append(best)
        # step 3
        survive = (cls_a != 1) & (blo <= best) & (blo < INF)
        out["outside_a"] += int((cls_a == 1).sum())
        out["pruned"] += int(((cls_a != 1) & ~survive).sum())
        depth_of = arr[:, 1]
        is_final = survive & (depth_of >= D)
        is_split = survive & (depth_of < D)
        if not finals and not survive.any():
            out.update(status=EMPTY, lo=INF, hi=INF)
            return out
        L = min([f[2] for f in finals] + [float(v) for v in blo[survive]])
        n_split = int(is_split.sum())
        if best - L <= tol:
            status = CONVERGED
        elif 8 * n_split > max_cells:
            status = CELL_LIMIT
        elif n_split == 0:
            status = DEPTH
        else:
            status = None
        nxt = []
        for i in np.nonzero(survive)[0]:
            node, depth, ci, cj, ck = cur[i]
            if status is None and is_split[i]:
                nxt += [(node, depth + 1, 2 * ci + (ch & 1), 2 * cj + ((ch >> 1) & 1), 2 * ck + (ch >> 2)) for ch in range(8)]
            else:
                finals.append((cur[i], int(cls_a[i]), float(blo[i])))
        if status is not None:
            out["status"] = status
            break
        cur = nxt
        level += 1
    out["hi"] = best
    out["lo"] = min(f[2] for f in finals)
    kept = [f for f in finals if not f[2] > best]
    out["pruned"] += len(finals) - len(kept)
    out["cells"] = [(c[0], c[1], cls, c[2], c[3], c[4]) for c, cls, _ in kept]
    if witness is not None:
        out["point"], out["image"], out["value_a"] = witness
    return out


def assert_equal(res, ref, what=None):
    """a product's Clearance (made with cells=True) against replay's dict: everything, exactly"""
    assert ref["ambiguous"] == 0, (what, "the replay met a cell whose class on A it cannot decide")
    assert (res.status, res.levels) == (ref["status"], ref["levels"]), (what, res, ref["status"], ref["levels"])
    assert (res.cells_visited, res.cells_outside_a, res.cells_pruned) == (ref["visited"], ref["outside_a"], ref["pruned"]), what
    assert res.cells_visited == sum(ref["lengths"]) and res.cells_open == len(ref["cells"]), what
    assert (res.lo, res.hi) == (ref["lo"], ref["hi"]), (what, res.lo, res.hi, ref["lo"], ref["hi"])
    if ref["point"] is None:
        assert np.isnan(res.point).all() and np.isnan(res.image).all() and np.isnan(res.value_a), what
    else:
        assert res.point.tobytes() == ref["point"].tobytes() and res.image.tobytes() == ref["image"].tobytes(), what
        assert res.value_a == ref["value_a"], what
    got = [(int(c["node"]), int(c["depth"]), int(c["cls"]), int(c["i"]), int(c["j"]), int(c["k"])) for c in res.cells]
    assert got == ref["cells"], (what, "the final cells")
