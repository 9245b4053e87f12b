"""A replay of QueryBounds (include/hpsdf.h, "QueryBounds"), written from the header's text and independent of the product's code.

What the header makes exactly reproducible is done in float64 with the stated expressions: the map of the two corners to the root's
frame, the float32 containment test, the child selection, the clip to [-(1 + E), 1 + E], the emptiness test, and the sub-boxes' l, h,
u_c and rho.  These decide `status` (but for NOT_FINITE) and `leaves`, which must therefore equal the product's exactly.  What the
header bounds instead of pinning -- f_c, G_a, S and e -- is computed in np.longdouble (64-bit mantissa) with tests/hiprec.py's
Legendre recurrence on tests/golden/ref_tables.npz.

The margin between the product's interval and this one, restated from the header's budget.  u = 2^-53.
  f_c    the recurrence errs by at most j^2 u <= 144 u per Legendre value (hiprec.py, (i)), three factors and the roundings of a term:
         under 2^-44 of a term; the 455-term sum in its fixed order adds 454 u of partial sums bounded by tau^3 S: under 2^-44 S more.
         The header charges 2^-41 S per evaluation; the long double value errs by 2^-11 of that.
  e      G_a and S are sums of up to 455 non-negative terms, each a product of four factors: relative error under 459 u < 2^-44; rho is
         exact here and there (the same float64 statements); the three products, two sums, the slack's multiplication, ETA * S and the
         last addition are 8 more roundings of non-negative quantities: under 2^-43 e in all.
  f_c -/+ e   rounded towards f_c: off by less than one spacing of doubles, 2 u (|f_c| + e) <= 2 u (1.03 S + e).
  lo is a minimum and hi a maximum over the same sub-boxes on both sides, and |min a_i - min b_i| <= max |a_i - b_i|.
So |lo - lo_ref| and |hi - hi_ref| stay under 2^-41 S_max + 2^-43 e_max + 2^-51 (S_max + e_max) < 2^-40 S_max + 2^-40 e_max, with
S_max the largest S over the leaves the box reached and e_max the largest e over its sub-boxes: the margin `margin()` returns.  No
constant here was taken from the code under test.
"""
import numpy as np

import hiprec as R

LD = R.LD
OK, LEAF_LIMIT, INVALID, NOT_FINITE = 0, 1, 2, 3
SLACK = 1.03125                    # HPSDF_SURFACE_SLACK
ETA = 2.0 ** -32                   # HPSDF_SURFACE_ETA
CLIP = 1.0 + 2.0 ** -14            # 1 + E


class Tree:
    """A serialised block as the walk sees it: children, degrees, coefficients, and per leaf G_0, G_1, G_2, S in long double."""

    def __init__(self, blk):
        B = blk if isinstance(blk, R.Block) else R.Block(blk)
        self.B = B
        self.rc = ((B.root_min + B.root_max) / np.float32(2.0)).astype(np.float64)
        self.inv = (np.float32(1.0) / (B.root_max - B.root_min)).astype(np.float64)
        self._consts = {}

    def consts(self, node, depth):
        if node not in self._consts:
            B = self.B
            deg = int(B.degree[node])
            nc = int(R.COUNT[deg])
            k = R.BIDX[:nc]
            nl = R.NL[:, depth].astype(LD)
            w = np.abs(B.coeffs[B.start[node]:B.start[node] + nc]).astype(LD) * nl[k[:, 0]] * nl[k[:, 1]] * nl[k[:, 2]]
            with np.errstate(invalid="ignore"):
                g = [(w * (k[:, a] * (k[:, a] + 1) // 2).astype(LD)).sum() for a in range(3)]
            self._consts[node] = (g[0], g[1], g[2], w.sum())
        return self._consts[node]

    def evaluate(self, node, depth, uc):
        """the leaf's polynomial at the rows of uc (float64 [m, 3]) in long double -> [m]"""
        B = self.B
        deg = int(B.degree[node])
        nc = int(R.COUNT[deg])
        k = R.BIDX[:nc]
        nl = R.NL[:deg + 1, depth].astype(LD)
        L = [R.legendre_ld(uc[:, a], deg) * nl[:, None] for a in range(3)]
        co = B.coeffs[B.start[node]:B.start[node] + nc].astype(LD)
        with np.errstate(invalid="ignore", over="ignore"):
            return (co[:, None] * L[0][k[:, 0]] * L[1][k[:, 1]] * L[2][k[:, 2]]).sum(0)


def _child_mask(pl, ph, c):
    out = []
    for i in range(8):
        ok = True
        for a in range(3):
            ok = ok and ((ph[a] >= c[a]) if (i >> a) & 1 else (pl[a] < c[a]))
        if ok:
            out.append(i)
    return out


def bounds_box(T, a, b, subdiv, max_leaves):
    """One box -> (lo, hi (long double), status, leaves, S_max, e_max (float))."""
    nan = LD(np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        pl = (np.asarray(a, np.float64) - T.rc) * T.inv
        ph = (np.asarray(b, np.float64) - T.rc) * T.inv
        fl, fh = pl.astype(np.float32), ph.astype(np.float32)
    half = np.float32(0.5)
    if not ((fl >= -half) & (fl <= half) & (fh >= -half) & (fh <= half) & (pl <= ph)).all():
        return nan, nan, INVALID, 0, 0.0, 0.0
    B = T.B
    state = {"lo": LD(np.inf), "hi": LD(-np.inf), "leaves": 0, "status": OK, "S": 0.0, "e": 0.0}
    part = 1.0 / subdiv
    m = np.arange(subdiv ** 3)
    shift = subdiv >> 1
    idx = np.stack([m & (subdiv - 1), (m >> shift) & (subdiv - 1), m >> (2 * shift)], 1)      # x fastest, then y, then z

    def visit(node, cen, depth):
        """the children of an interior node centred at cen (a node of depth `depth`)"""
        q = 0.25 / float(1 << depth)
        for i in _child_mask(pl, ph, cen):
            cc = np.array([cen[k] + q if (i >> k) & 1 else cen[k] - q for k in range(3)])
            ch = int(B.child[node]) + i
            ld = depth + 1
            if B.degree[ch] == R.INTERIOR:
                if not visit(ch, cc, ld):
                    return False
                continue
            if state["leaves"] == max_leaves:
                state["status"] = LEAF_LIMIT
                return False
            state["leaves"] += 1
            s = float(2 << ld)
            ua = np.maximum((pl - cc) * s, -CLIP)
            ub = np.minimum((ph - cc) * s, CLIP)
            if not (ua <= ub).all():
                continue
            w = (ub - ua) * part
            l = ua[None, :] + idx.astype(np.float64) * w[None, :]
            h = np.where(idx + 1 == subdiv, ub[None, :], ua[None, :] + (idx + 1).astype(np.float64) * w[None, :])
            uc, rho = 0.5 * (l + h), 0.5 * (h - l)
            g0, g1, g2, S = T.consts(ch, ld)
            with np.errstate(invalid="ignore", over="ignore"):
                fc = T.evaluate(ch, ld, uc)
                e = LD(SLACK) * ((rho[:, 0].astype(LD) * g0 + rho[:, 1].astype(LD) * g1) + rho[:, 2].astype(LD) * g2) + LD(ETA) * S
            if not (np.isfinite(fc).all() and np.isfinite(e).all()):
                state["status"] = NOT_FINITE
                return False
            state["lo"] = min(state["lo"], (fc - e).min())
            state["hi"] = max(state["hi"], (fc + e).max())
            state["S"] = max(state["S"], float(S))
            state["e"] = max(state["e"], float(e.max()))
        return True

    visit(0, np.zeros(3), 0)
    if state["status"] != OK:
        return LD(-np.inf), LD(np.inf), state["status"], state["leaves"], state["S"], state["e"]
    return state["lo"], state["hi"], OK, state["leaves"], state["S"], state["e"]


def bounds_reference(blk, boxes, subdiv=1, max_leaves=4096):
    """-> dict(lo, hi: long double [n]; status u8 [n]; leaves u32 [n]; S_max, e_max: float64 [n])."""
    T = blk if isinstance(blk, Tree) else Tree(blk)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    n = len(boxes)
    out = {"lo": np.empty(n, LD), "hi": np.empty(n, LD), "status": np.empty(n, np.uint8), "leaves": np.empty(n, np.uint32),
           "S_max": np.empty(n), "e_max": np.empty(n)}
    for i, row in enumerate(boxes):
        r = bounds_box(T, row[:3], row[3:], subdiv, max_leaves)
        for key, v in zip(("lo", "hi", "status", "leaves", "S_max", "e_max"), r):
            out[key][i] = v
    return out


def margin(ref):
    """the docstring's bound on |lo - lo_ref| and |hi - hi_ref| per box"""
    return 2.0 ** -40 * ref["S_max"] + 2.0 ** -40 * ref["e_max"]
