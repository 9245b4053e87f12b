"""A replay of IntegratePair's classification (include/hpsdf.h, "IntegratePair"), written from the header's text and independent of the
product's code, on tests/integrate_reference.py (A's class), tests/bounds_reference.py (the walk of B) and fractions.Fraction.

  * The image box: image_box(...) is the header's step 3 in float64, statement by statement in the header's association (Python floats
    are IEEE doubles and nothing is fused); exact_corner_images(...) gives the eight corners of the cell's exact box under the doubles M
    and t as Fractions, and sample_images(...) the float64 y of step 6 at the cell's corners and sub-box centres.
  * clamp(...) is step 4; class_b(...) steps 4 and 5 on bounds_reference.bounds_box, entered with the clamped range through a view of B
    whose root map is the identity; combine(...) and predicate(...) step 6.
  * replay_lists(...) runs the level loop over every list of a call and compares every cell's class, the order of the final cells and
    the list lengths with a product's result.  What the header bounds instead of pinning (f_c, e, lo, hi) is computed in np.longdouble;
    a cell within 2^-40 (S + e) of a threshold may fall on either side in float64, is reported as ambiguous and takes the product's class.
"""
import copy
from fractions import Fraction

import numpy as np

import bounds_reference as BR
import integrate_reference as IR

INTERSECTION, UNION, DIFFERENCE = 0, 1, 2
PMAX = 0.5 + 2.0 ** -25
PMIN = -PMAX
SLACK = 32.0 * 2.0 ** -53
LD = BR.LD


def root_map(root_min, root_max):
    """rootCentre and size = 1 / rootInvSizes as the library makes them from the float32 root box -> two lists of 3 floats"""
    rmin, rmax = np.asarray(root_min, np.float32), np.asarray(root_max, np.float32)
    centre = ((rmin + rmax) / np.float32(2.0)).astype(np.float64)
    inv = (np.float32(1.0) / (rmax - rmin)).astype(np.float64)
    return [float(v) for v in centre], [float(1.0 / v) for v in inv]


def deltas(centre, size, pose):
    out = []
    for j in range(3):
        m = pose[4 * j:4 * j + 3]
        X = [abs(centre[k]) + 0.5 * size[k] for k in range(3)]
        out.append(SLACK * (((abs(m[0]) * X[0] + abs(m[1]) * X[1]) + abs(m[2]) * X[2]) + abs(pose[4 * j + 3])))
    return out


def image(pose, x):
    """y = M x + t in the header's association"""
    return [((pose[4 * j] * x[0] + pose[4 * j + 1] * x[1]) + pose[4 * j + 2] * x[2]) + pose[4 * j + 3] for j in range(3)]


def image_box(centre, size, pose, depth, ijk, slack=True):
    """step 3 -> (a, b): two lists of 3 floats.  slack=False leaves delta out (the tests show that they can see it)."""
    s = 1.0 / float(1 << depth)
    cx, hx = [], []
    for k in range(3):
        pc = (-0.5 + float(ijk[k]) * s) + 0.5 * s
        cx.append(centre[k] + pc * size[k])
        hx.append((0.5 * s) * size[k])
    yc = image(pose, cx)
    d = deltas(centre, size, pose) if slack else [0.0] * 3
    a, b = [], []
    for j in range(3):
        m = pose[4 * j:4 * j + 3]
        r = (abs(m[0]) * hx[0] + abs(m[1]) * hx[1]) + abs(m[2]) * hx[2]
        rd = r + d[j]
        a.append(yc[j] - rd)
        b.append(yc[j] + rd)
    return a, b


def exact_corner_images(centre, size, pose, depth, ijk):
    """the eight corners of the exact box {centre + p size : p in the cell}, mapped exactly by the doubles M and t -> 8 x 3 Fractions"""
    s = Fraction(1, 1 << depth)
    F = Fraction
    out = []
    for corner in range(8):
        x = [F(centre[k]) + (F(-1, 2) + (ijk[k] + ((corner >> k) & 1)) * s) * F(size[k]) for k in range(3)]
        out.append([sum(F(pose[4 * j + k]) * x[k] for k in range(3)) + F(pose[4 * j + 3]) for j in range(3)])
    return out


def sample_images(centre, size, pose, depth, ijk, q=4):
    """the float64 y of step 6 at the cell's eight corners and its q^3 sub-box centres (p exact dyadics) -> list of [y0, y1, y2]"""
    s = 1.0 / float(1 << depth)
    plo = [-0.5 + float(ijk[k]) * s for k in range(3)]
    ps = [[plo[k] + ((c >> k) & 1) * s for k in range(3)] for c in range(8)]
    hs = 0.5 * (s * (1.0 / q))
    for n in range(q ** 3):
        idx = (n % q, (n // q) % q, n // (q * q))
        ps.append([plo[k] + float(2 * idx[k] + 1) * hs for k in range(3)])
    return [image(pose, [centre[k] + p[k] * size[k] for k in range(3)]) for p in ps]


def clamp(T, a, b):
    """step 4 -> (reach, pl, ph, partial): reach 0 walk, 1 no point of the box reaches B, 3 a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        pl = (np.asarray(a, np.float64) - T.rc) * T.inv
        ph = (np.asarray(b, np.float64) - T.rc) * T.inv
        fl, fh = pl.astype(np.float32), ph.astype(np.float32)
    if np.isnan(pl).any() or np.isnan(ph).any():
        return 3, pl, ph, True
    half = np.float32(0.5)
    if (fh < -half).any() or (fl > half).any():
        return 1, pl, ph, True
    low, high = ~(fl >= -half), ~(fh <= half)
    return 0, np.where(low, PMIN, pl), np.where(high, PMAX, ph), bool(low.any() or high.any())


def unit_view(T):
    """B with the identity as its root map: bounds_box(view, pl, ph, ...) then walks from the range [pl, ph] itself"""
    V = copy.copy(T)
    V.rc, V.inv = np.zeros(3), np.ones(3)
    return V


def class_b(T, V, a, b, iso_b, max_leaves):
    """steps 4 and 5 -> (class, ambiguous, status of the walk or None)"""
    reach, pl, ph, partial = clamp(T, a, b)
    if reach:
        return (1 if reach == 1 else 0), False, None
    lo, hi, status, _, S, e = BR.bounds_box(V, pl, ph, 1, max_leaves)
    assert status != BR.INVALID
    if status != BR.OK:
        return 0, False, status
    tol = LD(2.0 ** -40) * (LD(S) + LD(e))
    amb = bool(abs(lo - LD(iso_b)) <= tol or abs(hi - LD(iso_b)) <= tol)
    cls = 1 if lo > LD(iso_b) else (2 if (hi < LD(iso_b) and not partial) else 0)
    return cls, amb, status


def combine(op, ca, cb):
    if op == INTERSECTION:
        return 1 if 1 in (ca, cb) else (2 if ca == cb == 2 else 0)
    if op == UNION:
        return 1 if ca == cb == 1 else (2 if 2 in (ca, cb) else 0)
    return 1 if (ca == 1 or cb == 2) else (2 if (ca == 2 and cb == 1) else 0)


def predicate(op, in_a, in_b):
    return (in_a & in_b) if op == INTERSECTION else ((in_a | in_b) if op == UNION else (in_a & ~in_b))


def replay_lists(blk_a, blk_b, res, op, pose, iso_a, iso_b, D, max_leaves=256):
    """The level loop over every list of the call that gave `res` (made with cells=True and without a cell limit) ->
    dict(checked, ambiguous, wrong_class, walks, lengths); asserts that the final cells come in the product's order."""
    pose = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    rp = IR.Replay(blk_a)
    TB = BR.Tree(blk_b)
    VB = unit_view(TB)
    centre, size = root_map(rp.B.root_min, rp.B.root_max)
    product = {(int(c["node"]), int(c["depth"]), int(c["i"]), int(c["j"]), int(c["k"])): int(c["cls"]) for c in res.cells}
    split = set()
    for (node, depth, i, j, k) in product:
        for up in range(1, depth - int(rp.depth[node]) + 1):
            split.add((node, depth - up, i >> up, j >> up, k >> up))
    out = {"checked": 0, "ambiguous": 0, "wrong_class": 0, "walks": 0, "lengths": []}
    cur = [(int(n), int(rp.depth[n]), int(rp.ijk[n][0]), int(rp.ijk[n][1]), int(rp.ijk[n][2])) for n in rp.leaves]
    finals = []
    level = 0
    while cur:
        out["lengths"].append(len(cur))
        nxt = []
        for cell in cur:
            node, depth, i, j, k = cell
            assert (cell in product) != (cell in split), ("a cell of the replay's list is not the product's", cell)
            got = product.get(cell, 0)
            mask = (1 << level) - 1
            ca, amb = rp.classify(node, level, np.array([[i & mask, j & mask, k & mask]]), iso_a)
            ca, amb = int(ca[0]), bool(amb[0])
            if (ca == 2) if op == UNION else (ca == 1):
                cls = ca
            else:
                a, b = image_box(centre, size, pose, depth, (i, j, k))
                cb, amb_b, _ = class_b(TB, VB, a, b, iso_b, max_leaves)
                out["walks"] += 1
                cls, amb = combine(op, ca, cb), amb or amb_b
            out["checked"] += 1
            if amb:
                out["ambiguous"] += 1
            elif cls != got:
                out["wrong_class"] += 1
            if got == 0 and cell in split:
                assert depth < D
                nxt += [(node, depth + 1, 2 * i + (ch & 1), 2 * j + ((ch >> 1) & 1), 2 * k + (ch >> 2)) for ch in range(8)]
            else:
                assert got != 0 or depth >= D, ("an undecided cell above the depth limit was not split", cell)
                finals.append(cell + (got,))
        cur = nxt
        level += 1
    want = [(int(c["node"]), int(c["depth"]), int(c["i"]), int(c["j"]), int(c["k"]), int(c["cls"])) for c in res.cells]
    assert finals == want, "the final cells are not in list order, level by level"
    return out
