"""A replay of Integrate's classification (include/hpsdf.h, "Integrate"), written from the header's text and independent of the
product's code, on tests/hiprec.py and tests/bounds_reference.py's Tree.

What the header makes exactly reproducible is done in integers and float64: list 0 (the leaves in increasing node index, their depth
and integer coordinates from a walk of the children), a cell's box in its leaf's unit coordinates (lo = -1 + m 2^(1-l), hi = lo +
2^(1-l), u_c = 0.5 (lo + hi), rho = 2^-l: all exact).  What the header bounds instead of pinning -- f_c, G_a, S and e -- is computed in
np.longdouble.  A cell whose replayed | |f_c - iso| - e | is within bounds_reference.margin's bound, 2^-40 (S + e), can fall on either
side in float64 and is reported as ambiguous; every other cell's class must be the product's.

check_cells(blk, result, iso, D) applies the header's rule to a product's final cells:
  * a final cell's class equals the replay's;
  * every ancestor of a final cell inside its leaf (relative levels l - 1 .. 0) is undecided in the replay -- else it would not have been
    split;
  * an undecided final cell was not split for a stated reason: its depth is D, or its leaf is already at least that deep, or the call
    ended with CELL_LIMIT.
"""
import numpy as np

import bounds_reference as BR
import hiprec as R

LD = R.LD
OK, CELL_LIMIT, NOT_FINITE = 0, 1, 2


def leaf_cells(B):
    """List 0 from a walk of the children: (node, depth, i, j, k) rows in increasing node index."""
    n = len(B.degree)
    depth = np.full(n, -1, np.int64)
    ijk = np.zeros((n, 3), np.int64)
    depth[0] = 0
    stack = [0]
    while stack:
        p = stack.pop()
        if B.degree[p] != R.INTERIOR:
            continue
        first = int(B.child[p])
        for c in range(8):
            ch = first + c
            depth[ch] = depth[p] + 1
            ijk[ch] = 2 * ijk[p] + [(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1]
            stack.append(ch)
    lv = np.nonzero((B.degree != R.INTERIOR) & (depth >= 0))[0]
    return lv, depth, ijk


class Replay:
    def __init__(self, blk):
        self.T = BR.Tree(blk)
        self.B = self.T.B
        self.leaves, self.depth, self.ijk = leaf_cells(self.B)

    def classify(self, node, level, loc, iso):
        """cells of leaf `node` at relative level `level` with local integer coordinates loc [m, 3] -> (class [m], ambiguous [m])"""
        d = int(self.depth[node])
        w = 2.0 / float(1 << level)
        lo = -1.0 + loc.astype(np.float64) * w
        uc = 0.5 * (lo + (lo + w))
        rho = LD(1.0 / float(1 << level))
        g0, g1, g2, S = self.T.consts(node, d)
        with np.errstate(invalid="ignore", over="ignore"):
            fc = self.T.evaluate(node, d, uc)
            e = LD(BR.SLACK) * ((rho * g0 + rho * g1) + rho * g2) + LD(BR.ETA) * S
            diff = fc - LD(iso)
        cls = np.where(diff > e, 1, np.where(-diff > e, 2, 0)).astype(np.uint8)
        amb = np.abs(np.abs(diff) - e) <= LD(2.0 ** -40) * (S + e)
        return cls, np.asarray(amb, bool)


def check_cells(blk, res, iso, D):
    """-> dict(checked, ambiguous, wrong_class, decided_ancestor, unexplained): counts over the final cells of `res` and the ancestors of
    each level's cells."""
    rp = blk if isinstance(blk, Replay) else Replay(blk)
    cells = res.cells
    out = {"checked": 0, "ambiguous": 0, "wrong_class": 0, "decided_ancestor": 0, "unexplained": 0}
    for node in np.unique(cells["node"]):
        c = cells[cells["node"] == node]
        d = int(rp.depth[node])
        level = c["depth"].astype(np.int64) - d
        assert (level >= 0).all()
        abs_ijk = np.stack([c["i"], c["j"], c["k"]], 1).astype(np.int64)
        assert ((abs_ijk >> level[:, None]) == rp.ijk[node]).all(), "a cell outside its leaf"
        for l in np.unique(level):
            sel = level == l
            loc = abs_ijk[sel] & ((1 << int(l)) - 1)
            cls, amb = rp.classify(node, int(l), loc, iso)
            out["checked"] += int(sel.sum())
            out["ambiguous"] += int(amb.sum())
            out["wrong_class"] += int(((cls != c["cls"][sel]) & ~amb).sum())
            und = (c["cls"][sel] == 0) & ~amb
            explained = (c["depth"][sel] == D) | (d >= D) | (res.status == CELL_LIMIT)
            out["unexplained"] += int((und & ~explained).sum())
            # the ancestors of this level's cells, level by level up to the leaf itself
            anc = loc
            for up in range(int(l) - 1, -1, -1):
                anc = np.unique(anc >> 1, axis=0)
                acls, aamb = rp.classify(node, up, anc, iso)
                out["checked"] += len(anc)
                out["ambiguous"] += int(aamb.sum())
                out["decided_ancestor"] += int(((acls != 0) & ~aamb).sum())
    return out


def list_lengths(blk, res):
    """The lengths of lists 0 .. res.levels, from the final cells alone: list 0 holds the leaves, list l + 1 eight cells for every cell
    of list l that is not final."""
    rp = blk if isinstance(blk, Replay) else Replay(blk)
    level = res.cells["depth"].astype(np.int64) - rp.depth[res.cells["node"]]
    finals = np.bincount(level, minlength=res.levels + 1)
    lengths = [len(rp.leaves)]
    for l in range(res.levels):
        lengths.append(8 * (lengths[l] - int(finals[l])))
    assert lengths[-1] == finals[-1] and len(finals) == res.levels + 1
    return lengths
