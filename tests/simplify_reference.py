"""An extended-precision reference for Simplify (include/hpsdf.h, "Simplify"), independent of the product: the transfer matrices from
their integral in exact rational arithmetic, the merge, its residual, the bound and the truncation in np.longdouble, the whole rule
replayed over a block, and a distance between two blocks that uses no transfer matrix at all.  The reference's numbers come only from
tests/golden/ref_tables.npz, through hiprec (coeff_count[6] == 83, rows in basis_index order).

Notation as in hiprec.py: u = 2^-53, fl(a op b) = (a op b)(1 + d) with |d| <= u, first-order bounds times SLACK = 1 + 1e-6.

1. Tables.  P_i((t + 2s - 1) / 2) P_j(t) is a polynomial with rational coefficients, so its integral over [-1, 1] is a rational R, found
   here with fractions.Fraction: no quadrature, no rounding.  T = sqrt((2i+1)(2j+1)/2) * R / 2 is then formed in long double: the square
   root of an exactly representable number (relative 2^-64), R to within 2^-70 absolute, two multiplications: far inside half an ulp of
   a double.  The product's table must lie within 1 ulp (of the exact value's double) of it, and be exactly 0 where R = 0 and above the
   diagonal.  sum_s T_s T_s^T = I for the real matrices; for tables within 1 ulp (relative 2u) of them every entry of the sum moves by
   at most sum_k 2 * 2u |T_s[i][k] T_s[j][k]| <= 4u (rows of the real matrices have norm <= 1), and the float64 matrix product adds
   26 roundings of terms of the same size: |sum_s T_s T_s^T - I| <= 30 u.

2. The merge.  Every entry of the image of a child is three nested dot products of at most 13 terms; a term of a dot product passes
   through one multiplication and at most 13 additions, and its T carries 2u (the tables, section 1): 16 u a pass, 48 u for three, and
   8 more roundings for the sum over the children: K_FWD = 56.  With |T| the matrices of absolute values and dc_n >= |the rows the
   product holds - the rows the replay holds| (0 for a leaf of the source),
       |parent - parent*| <= dP := K_FWD u A(|c_n| + dc_n) + A(dc_n),   A(x) = sum_n |T_sx| |T_sy| |T_sz| x_n  (the same three passes).
   The restriction is three passes again, K_BWD = 48:  |r_n - r_n*| <= dr_n := K_BWD u B_n(|parent*| + dP) + B_n(dP), B_n the
   restriction with |T|.  d = fl(c_n - r_n): dd := dr_n + dc_n + u (|d*| + dr_n + dc_n).  The squares: one rounding each, 8 additions
   over the children, at most 9 steps of the reduction tree: K_SUM = 18.
       |e_step - e_step*| <= de := sum (2 |d*| dd + dd^2) + K_SUM u sum (|d*| + dd)^2.
   For children that ARE restrictions of one parent d* is rounding (u |c|), so e_step <= de ~ (K u)^2 |c|^2 with K ~ 150: the product
   of two rounding errors, as it must be.  (sum |c_n|^2 - |parent|^2 would carry u |c|^2 instead: 1e13 times more.)
   sqrt: |sqrt(x) - sqrt(x*)| <= min(sqrt(dx), dx / sqrt(x*)) + u sqrt(x*); the sum of the children's e: de_n and 8 roundings;
   r = s + t: + u r; b = r^2: db = 2 r dr + dr^2 + u b.  A decision is in doubt iff |b* - threshold| <= db (the threshold, (rms rms) vol,
   is one rounding of a number the replay forms the same way: 2u of it is added to db).

3. Truncation.  tail = sum of squares of rows that carry dc: |tail - tail*| <= sum (2 |c*| dc + dc^2) + (rows + 1) u sum (|c*| + dc)^2,
   then the bound as in 2.

4. l2_distance.  Source leaf by source leaf: (result - source)^2 is a polynomial of degree <= 2 max(deg) per axis, for which the
   Gauss rule of max(deg) + 1 nodes is exact; both polynomials are evaluated at the nodes by hiprec's series in long double.  The
   golden nodes and weights are doubles (relative u): with g the integrand, the sum moves by at most u sum w (3 |g| + |dg/dx|): both
   are bounded by (1 + 2 * 12^2) times the integral of a polynomial's square on the scale of (|result| + |source|)^2, i.e. 300 u E_C with
   E_C the energy of the two fields over the cell.  This enters the guarantee's slack below.

5. The guarantee's slack.  The product's e is its float64 e_step, wrong by de (section 2) -- relative to the ENERGY E_C of the source over
   the cell, not to e: de <= 2 K u sqrt(e E_C) + (K u)^2 E_C with K = K_FWD + K_BWD + K_SUM per level, L levels.  So a cell's true
   deviation may exceed rms^2 vol by K_G u (sqrt(rms^2 vol E_C) + E_C u K_G), K_G = 2 L (K_FWD + K_BWD + K_SUM) + 300:
       slack_C = K_G u (sqrt(E_C / (rms^2 vol)) + 1) + (K_G u)^2 E_C / (rms^2 vol).
   Nothing here was chosen by looking at the product's output.
"""
from fractions import Fraction

import numpy as np

import hiprec as HR
from hiprec import LD, U, SLACK, COUNT, BIDX, NL, INTERIOR

K_FWD, K_BWD, K_SUM = 56, 48, 18
MERGE, TRUNCATE = 1, 2


# ------------------------------------------------------------------------------------------------------------------ tables
def _legendre_polys(n):
    """P_0 .. P_n as coefficient lists (Fractions, ascending powers)."""
    P = [[Fraction(1)], [Fraction(0), Fraction(1)]]
    for k in range(2, n + 1):
        a = [Fraction(0)] + [Fraction(2 * k - 1, k) * c for c in P[k - 1]]
        b = [Fraction(k - 1, k) * c for c in P[k - 2]] + [Fraction(0)] * 2
        P.append([x - y for x, y in zip(a, b)])
    return P[:n + 1]


def _poly_mul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def _compose_half(p, s):
    """p((t + 2s - 1) / 2) as a polynomial in t."""
    x = [Fraction(2 * s - 1, 2), Fraction(1, 2)]
    out, pw = [Fraction(0)], [Fraction(1)]
    for c in p:
        out = [a + b for a, b in zip(out + [Fraction(0)] * (len(pw) - len(out)), [c * v for v in pw])]
        pw = _poly_mul(pw, x)
    return out


def _frac_to_ld(fr):
    """A Fraction of magnitude below 2^20 as a long double, to within 2^-70 absolute."""
    k = (abs(fr.numerator) << 70) // fr.denominator
    out = LD(0)
    for shift in (60, 30, 0):
        out += LD(float((k >> shift) & ((1 << 30) - 1))) * LD(2.0) ** (shift - 70)
    out += LD(float(k >> 90)) * LD(2.0) ** 20
    return -out if fr < 0 else out


_TABLES = None


def transfer_tables():
    """(T long double [2, 13, 13], exact-zero mask [2, 13, 13]) from the integral (docstring, section 1)."""
    global _TABLES
    if _TABLES is None:
        P = _legendre_polys(12)
        T = np.zeros((2, 13, 13), LD)
        zero = np.ones((2, 13, 13), bool)
        for s in range(2):
            comp = [_compose_half(P[i], s) for i in range(13)]
            for i in range(13):
                for j in range(i + 1):
                    prod = _poly_mul(comp[i], P[j])
                    R = sum((c * Fraction(2, m + 1) for m, c in enumerate(prod) if m % 2 == 0), Fraction(0))
                    if R != 0:
                        zero[s, i, j] = False
                        T[s, i, j] = np.sqrt(LD((2 * i + 1) * (2 * j + 1)) / LD(2)) * LD(0.5) * _frac_to_ld(R)
        _TABLES = (T, zero)
    return _TABLES


def transfer_f64():
    """The tables rounded to double: what the rule's statements are fed with."""
    return transfer_tables()[0].astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ cubes
def rows_to_cube(rows, deg, Q):
    """rows [..., >= COUNT[deg]] of a polynomial of degree `deg` -> dense [..., Q, Q, Q]; entries not stored are 0."""
    nc = int(COUNT[deg])
    cube = np.zeros(rows.shape[:-1] + (Q, Q, Q), rows.dtype)
    cube[..., BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]] = rows[..., :nc]
    return cube


def cube_to_rows(cube, deg):
    nc = int(COUNT[deg])
    return cube[..., BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]]


def _stored_mask(q, Q):
    m = np.zeros((Q, Q, Q), bool)
    nc = int(COUNT[q])
    m[BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]] = True
    return m


def _halves(n):
    return n & 1, (n >> 1) & 1, (n >> 2) & 1


def project(T, cubes):
    """cubes [N, 8, Q, Q, Q] (children 0 .. 7) -> their image in the parent [N, Q, Q, Q] (all entries; mask afterwards)."""
    Q = cubes.shape[-1]
    out = np.zeros(cubes.shape[:1] + (Q, Q, Q), cubes.dtype)
    for n in range(8):
        sx, sy, sz = _halves(n)
        out += np.einsum("ai,bj,ck,Nijk->Nabc", T[sx][:Q, :Q], T[sy][:Q, :Q], T[sz][:Q, :Q], cubes[:, n])
    return out


def restrict(T, parent, n):
    """parent [N, Q, Q, Q] -> its polynomial over child n, [N, Q, Q, Q]."""
    Q = parent.shape[-1]
    sx, sy, sz = _halves(n)
    return np.einsum("ai,bj,ck,Nabc->Nijk", T[sx][:Q, :Q], T[sy][:Q, :Q], T[sz][:Q, :Q], parent)


def _sqrt_err(x, dx):
    """|sqrt(x~) - sqrt(x)| for |x~ - x| <= dx, x >= 0, plus the rounding of the root."""
    x, dx = np.asarray(x, np.float64), np.asarray(dx, np.float64)
    root = np.sqrt(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(root > 0, dx / root, np.inf)
    return np.minimum(np.sqrt(dx), lin) + U * (root + np.sqrt(dx))


def bound_with_error(step, dstep, carried, dcarried):
    """b = (sqrt(step) + sqrt(carried))^2 in long double and the bound on the product's deviation from it (section 2)."""
    s, t = np.sqrt(step), np.sqrt(carried)
    r = s + t
    dr = _sqrt_err(step, dstep) + _sqrt_err(carried, dcarried) + U * r.astype(np.float64)
    b = r * r
    db = (2 * r.astype(np.float64) * dr + dr * dr + U * b.astype(np.float64)) * SLACK
    return b, db


def merge_group(T, Tabs, rows, drows, degs, q, e, de):
    """Candidates of one degree q: rows [N, 8, COUNT[q]] long double (zero-padded), drows their error bounds (float64), degs [N, 8],
    e / de [N, 8] -> dict(parent rows, dparent, e_step, de_step, b, db)."""
    Q = q + 1
    N = rows.shape[0]
    cubes = np.zeros((N, 8, Q, Q, Q), LD)
    dcubes = np.zeros((N, 8, Q, Q, Q))
    for d in np.unique(degs):
        sel = degs == d
        cubes[sel] = rows_to_cube(rows[sel], int(d), Q)
        dcubes[sel] = rows_to_cube(drows[sel], int(d), Q)
    mask = _stored_mask(q, Q)
    parent = project(T, cubes) * mask
    acubes = np.abs(cubes).astype(np.float64)
    dP = (K_FWD * U * project(Tabs, acubes + dcubes) + project(Tabs, dcubes)) * mask * SLACK
    aP = np.abs(parent).astype(np.float64)
    step, dstep = np.zeros(N, LD), np.zeros(N)
    for n in range(8):
        d = cubes[:, n] - restrict(T, parent, n)
        dr = K_BWD * U * restrict(Tabs, aP + dP, n) + restrict(Tabs, dP, n)
        ad = np.abs(d).astype(np.float64)
        dd = dr + dcubes[:, n] + U * (ad + dr + dcubes[:, n])
        step += (d * d).sum((1, 2, 3))
        dstep += (2 * ad * dd + dd * dd).sum((1, 2, 3)) + K_SUM * U * ((ad + dd) ** 2).sum((1, 2, 3))
    dstep *= SLACK
    carried = e.sum(1)
    dcarried = de.sum(1) + 8 * U * carried.astype(np.float64)
    b, db = bound_with_error(step, dstep, carried, dcarried)
    return {"rows": cube_to_rows(parent, q), "drows": cube_to_rows(dP, q), "e_step": step, "de_step": dstep, "b": b, "db": db}


def truncate_leaf(rows, drows, deg, e, de, thr):
    """One leaf: -> (new degree, e, de, [(degree tried, b, db)])."""
    a = np.abs(rows).astype(np.float64)
    tried, keep, eo, deo = [], deg, e, de
    for dd in range(deg - 1, -1, -1):
        lo = int(COUNT[dd])
        tail = (rows[lo:] * rows[lo:]).sum()
        dtail = ((2 * a[lo:] * drows[lo:] + drows[lo:] ** 2).sum() + (len(rows) - lo + 1) * U * ((a[lo:] + drows[lo:]) ** 2).sum()) * SLACK
        b, db = bound_with_error(tail, dtail, e, de)
        tried.append((dd, b, float(db)))
        if not (b <= thr and np.isfinite(b)):
            break
        keep, eo, deo = dd, b, float(db)
    return keep, eo, deo, tried


# ------------------------------------------------------------------------------------------------------------------ the rule replayed
def volume(depth):
    return LD(1) / LD(8) ** int(depth)


def tree_depths(blk):
    """Path length from the root per node (-1: not reached), by a walk."""
    depth = np.full(len(blk.degree), -1, np.int64)
    depth[0] = 0
    stack = [0]
    while stack:
        i = stack.pop()
        if blk.degree[i] == INTERIOR:
            c = int(blk.child[i])
            depth[c:c + 8] = depth[i] + 1
            stack.extend(range(c, c + 8))
    return depth


def replay(block, rms, flags=MERGE | TRUNCATE):
    """The rule over a block in long double -> dict:
         degree [nodes]    the final degree (13: interior; -1: dropped or never reached)
         merged            set of the nodes whose merge was accepted
         rows, drows       per surviving leaf: its long-double rows and the bound on the product's deviation from them
         e, de             per surviving leaf
         merge_doubt       {node: True} for candidates whose b lies within db of the threshold
         trunc_doubt       {leaf: True} for leaves where a truncation step's b does
         decisions         the number of decisions taken (candidates + truncation steps)"""
    blk = block if isinstance(block, HR.Block) else HR.Block(block)
    T = transfer_f64().astype(LD)
    Tabs = np.abs(transfer_f64())
    nn = len(blk.degree)
    depth = tree_depths(blk)
    degree = np.where(depth >= 0, blk.degree, -1).astype(np.int64)
    rows, drows, e, de = {}, {}, {}, {}
    for i in np.nonzero((degree >= 0) & (degree != INTERIOR))[0]:
        nc = int(COUNT[degree[i]])
        rows[i] = blk.coeffs[blk.start[i]:blk.start[i] + nc].astype(LD)
        drows[i] = np.zeros(nc)
        e[i], de[i] = LD(0), 0.0
    out = {"merged": set(), "merge_doubt": {}, "trunc_doubt": {}, "decisions": 0}
    rms2 = LD(float(rms) * float(rms))   # the threshold's first factor is the product's own double
    if rms > 0 and flags & MERGE:
        for D in range(int(depth.max()), 1, -1):
            cands = [i for i in np.nonzero((depth == D - 1) & (degree == INTERIOR))[0]
                     if all(degree[int(blk.child[i]) + n] != INTERIOR for n in range(8))]
            if not cands:
                continue
            qs = np.array([max(degree[int(blk.child[i]) + n] for n in range(8)) for i in cands])
            thr = rms2 * volume(D - 1)
            for q in np.unique(qs):
                grp = [i for i, qq in zip(cands, qs) if qq == q]
                nc = int(COUNT[q])
                R, dR = np.zeros((len(grp), 8, nc), LD), np.zeros((len(grp), 8, nc))
                G, E, dE = np.zeros((len(grp), 8), np.int64), np.zeros((len(grp), 8), LD), np.zeros((len(grp), 8))
                for k, i in enumerate(grp):
                    for n in range(8):
                        c = int(blk.child[i]) + n
                        R[k, n, :len(rows[c])], dR[k, n, :len(rows[c])] = rows[c], drows[c]
                        G[k, n], E[k, n], dE[k, n] = degree[c], e[c], de[c]
                m = merge_group(T, Tabs, R, dR, G, int(q), E, dE)
                for k, i in enumerate(grp):
                    b, db = m["b"][k], float(m["db"][k]) + 2 * U * float(thr)
                    out["decisions"] += 1
                    if abs(float(b - thr)) <= db:
                        out["merge_doubt"][int(i)] = True
                    if b <= thr and np.isfinite(b):
                        out["merged"].add(int(i))
                        degree[i] = q
                        rows[i], drows[i], e[i], de[i] = m["rows"][k], m["drows"][k], b, float(m["db"][k])
                        c = int(blk.child[i])
                        for n in range(8):
                            degree[c + n] = -1
                            for t in (rows, drows, e, de):
                                t.pop(c + n)
    if rms > 0 and flags & TRUNCATE:
        for i in sorted(rows):
            if degree[i] == 0:
                continue
            thr = rms2 * volume(depth[i])
            keep, eo, deo, tried = truncate_leaf(rows[i], drows[i], int(degree[i]), e[i], de[i], thr)
            out["decisions"] += len(tried)
            if any(abs(float(b - thr)) <= db + 2 * U * float(thr) for _, b, db in tried):
                out["trunc_doubt"][int(i)] = True
            if keep != degree[i]:
                nc = int(COUNT[keep])
                degree[i], rows[i], drows[i], e[i], de[i] = keep, rows[i][:nc], drows[i][:nc], eo, deo
    # dropped sub-trees below a merged node: everything under it
    alive = np.zeros(nn, bool)
    stack = [0]
    while stack:
        i = stack.pop()
        alive[i] = True
        if degree[i] == INTERIOR:
            stack.extend(range(int(blk.child[i]), int(blk.child[i]) + 8))
    degree[~alive] = -1
    out.update(degree=degree, rows=rows, drows=drows, e=e, de=de, depth=depth, block=blk)
    return out


def result_leaves(source, result):
    """The result's leaves by the SOURCE's node index: the surviving nodes keep their order, so the k-th surviving source node is the
    result's node k.  -> (source index per result node, Block of the result)."""
    src = source if isinstance(source, HR.Block) else HR.Block(source)
    res = result if isinstance(result, HR.Block) else HR.Block(result)
    # walk both trees together: a result node is interior only where the source node is
    pair = np.full(len(res.degree), -1, np.int64)
    stack = [(0, 0)]
    while stack:
        s, r = stack.pop()
        pair[r] = s
        if res.degree[r] == INTERIOR:
            assert src.degree[s] == INTERIOR, "the result splits a cell the source does not"
            for n in range(8):
                stack.append((int(src.child[s]) + n, int(res.child[r]) + n))
    return pair, res


# ------------------------------------------------------------------------------------------------------------------ distance
def _eval_cubes(coeff_cubes, depth, x):
    """Polynomials [N, Q, Q, Q] at depth `depth` (int [N]) at unit coordinates x [N, 3, n] -> values on the tensor grid [N, n, n, n]."""
    Q = coeff_cubes.shape[-1]
    LN = []
    for a in range(3):
        L = HR.legendre_ld(x[:, a, :].reshape(-1), Q - 1).reshape(Q, x.shape[0], x.shape[2])   # [Q, N, n]
        LN.append(L * NL[:Q, depth].astype(LD)[:, :, None])
    return np.einsum("Nabc,aNx,bNy,cNz->Nxyz", coeff_cubes, LN[0], LN[1], LN[2])


def l2_distance(source, result):
    """The integral of (result - source)^2 over the root in the root-normalised frame, source leaf by source leaf (docstring, section 4)
    -> (total, per-result-leaf sums {result node: sum}, per-result-leaf source energy {result node: sum of the source rows' squares})."""
    src = source if isinstance(source, HR.Block) else HR.Block(source)
    res = result if isinstance(result, HR.Block) else HR.Block(result)
    sdepth, rdepth = tree_depths(src), tree_depths(res)
    sl = np.nonzero((sdepth >= 0) & (src.degree != INTERIOR))[0]
    cen = ((src.bmin[sl] + src.bmax[sl]) / np.float32(2.0)).astype(np.float64)       # exact dyadics
    rl = res.descend(cen)
    per, energy = {}, {}
    total = LD(0)
    key = ((src.degree[sl] * 16 + sdepth[sl]) * 16 + res.degree[rl]) * 16 + rdepth[rl]
    for k in np.unique(key):
        sel = np.nonzero(key == k)[0]
        sdeg, sdep, rdeg, rdep = int(k) >> 12, (int(k) >> 8) & 15, (int(k) >> 4) & 15, int(k) & 15
        n = max(sdeg, rdeg) + 1
        xs, ws = HR.rule(n)
        s_nodes, r_nodes = sl[sel], rl[sel]
        sc = src.coeffs[src.start[s_nodes][:, None] + np.arange(int(COUNT[sdeg]))[None, :]].astype(LD)
        rc = res.coeffs[res.start[r_nodes][:, None] + np.arange(int(COUNT[rdeg]))[None, :]].astype(LD)
        x_src = np.broadcast_to(xs[None, None, :], (len(sel), 3, n))
        # the nodes in the root's frame (exact: dyadic centre + node * 2^-(d+1) has at most 53 + 11 bits; formed in long double)
        p = cen[sel][:, :, None].astype(LD) + xs.astype(LD)[None, None, :] * LD(2.0) ** (-(sdep + 1))
        rcen = ((res.bmin[r_nodes] + res.bmax[r_nodes]) / np.float32(2.0)).astype(np.float64)
        x_res = (p - rcen[:, :, None].astype(LD)) * LD(2.0) ** (rdep + 1)
        fs = _eval_cubes(rows_to_cube(sc, sdeg, sdeg + 1), np.full(len(sel), sdep), x_src)
        fr = _eval_ld_cubes(rows_to_cube(rc, rdeg, rdeg + 1), np.full(len(sel), rdep), x_res)
        w = ws.astype(LD)
        g = (fr - fs) ** 2
        cell = np.einsum("Nxyz,x,y,z->N", g, w, w, w) * (volume(sdep) / LD(8))
        for j, r in enumerate(r_nodes):
            per[int(r)] = per.get(int(r), LD(0)) + cell[j]
            energy[int(r)] = energy.get(int(r), LD(0)) + (sc[j] * sc[j]).sum()
        total += cell.sum()
    return total, per, energy


def _eval_ld_cubes(coeff_cubes, depth, x):
    """_eval_cubes for coordinates that are already long double (the result leaf's, which need not be doubles)."""
    Q = coeff_cubes.shape[-1]
    LN = []
    for a in range(3):
        xa = x[:, a, :]
        L = np.empty((Q,) + xa.shape, LD)
        m2, m1 = np.zeros_like(xa), np.ones_like(xa)
        L[0] = 1
        for j in range(1, Q):
            li = LD(HR.REC[j][0]) * xa * m1 - LD(HR.REC[j][1]) * m2
            m2, m1 = m1, li
            L[j] = li
        LN.append(L * NL[:Q, depth].astype(LD)[:, :, None])
    return np.einsum("Nabc,aNx,bNy,cNz->Nxyz", coeff_cubes, LN[0], LN[1], LN[2])


def guarantee_slack(energy, rms, vol, levels):
    """slack_C of section 5 for a cell with source energy E_C."""
    kg = 2 * max(1, levels) * (K_FWD + K_BWD + K_SUM) + 300
    ratio = float(energy) / (float(rms) ** 2 * float(vol))
    return kg * U * (np.sqrt(ratio) + 1.0) + (kg * U) ** 2 * ratio


# ------------------------------------------------------------------------------------------------------------------ test blocks
def exact_merge_block(rng, parent_degrees, child_degree, depth1_only=False):
    """A depth-2 block -- the root, 8 interior children, 64 leaves -- whose eight leaves under child p are the long-double restrictions,
    rounded to double, of one random parent of degree parent_degrees[p], stored at degree child_degree (zero tails above the parent's).
    -> (block bytes, parents long double [8][COUNT[parent degree]])."""
    T = transfer_tables()[0]
    Q = child_degree + 1
    parents, leaves = [], []
    for p in range(8):
        dp = parent_degrees[p]
        rows = rng.standard_normal(int(COUNT[dp])).astype(LD)
        parents.append(rows)
        cube = rows_to_cube(rows[None, :], dp, Q)
        for n in range(8):
            leaves.append(cube_to_rows(restrict(T, cube, n), child_degree)[0].astype(np.float64))
    return make_depth2_block(leaves, [child_degree] * 64), parents


def make_depth2_block(leaf_rows, leaf_degrees, root_min=(-0.5,) * 3, root_max=(0.5,) * 3):
    """The root, 8 interior children (nodes 1 .. 8), and their 64 leaves (child p's at 9 + 8 p ..) with the given rows."""
    def node(child, bmin, bmax, start, degree, dep):
        b = np.zeros(56, np.uint8)
        b[0:8] = np.array([child], np.uint64).view(np.uint8)
        b[8:32] = np.array(list(bmin) + list(bmax), np.float32).view(np.uint8)
        b[32:40] = np.array([start], np.uint64).view(np.uint8)
        b[40] = degree
        b[48] = dep
        return b

    def corner(bmin, bmax, i):
        lo, hi = list(bmin), list(bmax)
        for d in range(3):
            mid = (np.float32(bmax[d]) + np.float32(bmin[d])) * np.float32(0.5)
            if (i >> d) & 1:
                lo[d] = mid
            else:
                hi[d] = mid
        return lo, hi

    leaf = np.uint64(0xFFFFFFFFFFFFFFFF)
    rmin, rmax = [-0.5] * 3, [0.5] * 3
    nodes = [node(1, rmin, rmax, 0, 13, 0)]
    boxes = [corner(rmin, rmax, p) for p in range(8)]
    for p in range(8):
        nodes.append(node(9 + 8 * p, boxes[p][0], boxes[p][1], 0, 13, 1))
    # coefficients in the canonical order: a depth-first walk, children 0 .. 7 -- child p's leaves follow child p - 1's
    cur = 0
    for p in range(8):
        for n in range(8):
            lo, hi = corner(boxes[p][0], boxes[p][1], n)
            nodes.append(node(leaf, lo, hi, cur, leaf_degrees[8 * p + n], 2))
            cur += len(leaf_rows[8 * p + n])
    coeffs = np.concatenate([np.asarray(r, np.float64) for r in leaf_rows])
    cfg = np.zeros(80, np.uint8)
    cfg[40:48] = np.array([1e-10], np.float64).view(np.uint8)
    cfg[48:56] = np.array([1], np.uint64).view(np.uint8)
    cfg[56:80] = np.array(list(root_min) + list(root_max), np.float32).view(np.uint8)
    return (np.array([len(coeffs)], np.uint64).tobytes() + coeffs.tobytes() + np.array([len(nodes)], np.uint64).tobytes()
            + np.concatenate(nodes).tobytes() + cfg.tobytes())
