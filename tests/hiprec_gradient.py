"""An extended-precision reference for QueryGradient (include/hpsdf.h; csrc/leaf_jet.hpp) on top of hiprec.Block, and a
worst-case bound per gradient component derived from the order of the operations, in the manner of hiprec.py section 3.

What the product forms in float64 before the arithmetic under test -- the root remap (hiprec.Block.to_unit), the descent
(Block.descend) and the leaf's unit coordinates x = (q - centre) * (2 << d) -- is reproduced bit for bit in numpy; everything after
it runs in np.longdouble.  u = 2^-53; bounds are first order and multiplied by hiprec.SLACK.  No constant was chosen by looking at
the implementation's output.

The operation, per leaf (degree p, depth d, coefficients c_i in basis order (a, b, c), N_j = normalised_lengths[j][d]):
    L_j(x)   by Query's recurrence;   D_0 = 0, D_1 = 1, D_j = fl(D_{j-2} + fl((2j-1) L_{j-1}));   LN_j = fl(L_j N_j), DN_j = fl(D_j N_j)
    gu_0 = sum_i fl(c_i fl(fl(DN_a(x) LN_b(y)) LN_c(z)))  in the loop's fixed order from 0.0;  gu_1, gu_2 with D on the other axes
    g_k  = fl(fl(gu_k 2^(d+1)) inv_k),  inv_k the float64 widening of the tree's float32 reciprocal root size (exact input)

Error sources for component 0 (the others by symmetry), |x|, |y|, |z| <= 1:
  (i)   the recurrence: |dL_j| <= j^2 u (hiprec section 2 (i), checked by test_recurrence_error_model).
  (ii)  the derivative's own accumulation.  D_j is a sum of at most ceil(j/2) terms (2k+1) L_k, k = j-1, j-3, ...; each term carries
        the recurrence error of its L_k scaled by (2k+1), one product rounding u (2k+1) |L_k|, and each partial sum D_m, m = j, j-2,
        ... >= 2, one addition rounding u |D_m| (for even j the first addition, to D_0 = 0, is exact; it is counted all the same):
            |dD_j| <= u eD_j,   eD_j = sum_{k = j-1, j-3, .. >= 0} (2k+1) (k^2 + |L_k|)  +  sum_{m = j, j-2, .. >= 2} |D_m|,  eD_0 = eD_1 = 0.
  (iii) per term: DN, LN, LN one rounding each (3), the two products (2), c_i times the product (1): K_G = 6 roundings on
        |c_i| N_a N_b N_c |D_a L_b L_c|.
  (iv)  the running sum: u sum_{i >= 1} |s_i| with s_i the exact partial sums (the addition to 0.0 is exact).
  So  |dgu_0| <= u ( sum_i |c_i| N_a N_b N_c ( eD_a |L_b L_c| + b^2 |D_a L_c| + c^2 |D_a L_b| + K_G |D_a L_b L_c| ) + sum_{i>=1} |s_i| ).
  (v)   the world scaling: two roundings (the first is by a power of two and in fact exact): |dg_k| <= |dgu_k| 2^(d+1) inv_k + 2u |g_k|.
  (vi)  HPSDF_GRADIENT_UNIT, as hiprec treats normalize(): the map g -> g/|g| has Jacobian norm 1/|g|, and z = sum3(g^2) (3u, either
        order), the square root (2.5u) and the division (3.5u in all) add 3.5u per component:  |v_k - v*_k| <= |dg|_2 / |g*| + 3.5u.
"""
import numpy as np

import hiprec as R

LD = R.LD
K_G = 6


def derivative_ld(L, p, scale=None):
    """D_0..D_p from L_0..L_p (long double, [p + 1]) by the stated recurrence.  scale: {j: factor on the constant (2j-1)} (mutants)."""
    D = np.zeros(p + 1, LD)
    if p >= 1:
        D[1] = 1
    for j in range(2, p + 1):
        k = LD(2 * j - 1) * (LD(scale[j]) if scale and j in scale else LD(1))
        D[j] = D[j - 2] + k * L[j - 1]
    return D


def derivative_error_units(Labs, Dabs, p):
    """eD_j of (ii), j = 0..p, from |L_k| and |D_m| (float64)."""
    e = np.zeros(p + 1)
    for j in range(2, p + 1):
        e[j] = sum((2 * k + 1) * (k * k + Labs[k]) for k in range(j - 1, -1, -2)) + sum(Dabs[m] for m in range(j, 1, -2))
    return e


def gradient_reference(block, points, left=False, dscale=None, leaf=None):
    """QueryGradient of a MemoryBlock at world points inside the root -> dict(f, g [n,3] long double and g_bound [n,3]: the world
    gradient; n, n_bound: the row under HPSDF_GRADIENT_UNIT (left: the reduction order); gu: the unit-space partials; leaf).
    leaf: evaluate from these leaves instead of the descent's (the unit coordinates then refer to those leaves' centres): mutants."""
    blk = block if isinstance(block, R.Block) else R.Block(block)
    q = blk.to_unit(points)
    leaf = blk.descend(q) if leaf is None else np.asarray(leaf)
    inv = (np.float32(1.0) / (blk.root_max - blk.root_min)).astype(np.float64)
    npt = len(q)
    f = np.empty(npt, LD)
    g, gb = np.zeros((npt, 3), LD), np.zeros((npt, 3))
    gn, gnb = np.zeros((npt, 3), LD), np.zeros((npt, 3))
    gu = np.zeros((npt, 3), LD)
    for i in range(npt):
        n = leaf[i]
        deg, dep = int(blk.degree[n]), int(blk.depth[n])
        cen = ((blk.bmin[n] + blk.bmax[n]) / np.float32(2.0)).astype(np.float64)
        x = (q[i] - cen) * float(2 << dep)                   # Octree.cpp:862, float64
        nc = int(R.COUNT[deg])
        co = blk.coeffs[blk.start[n]:blk.start[n] + nc]
        idx = [R.BIDX[:nc, k] for k in range(3)]
        Nd = R.NL[:deg + 1, dep].astype(LD)
        L = [R.legendre_ld(np.array([x[k]]), deg)[:, 0] for k in range(3)]
        D = [derivative_ld(L[k], deg, dscale) for k in range(3)]
        Lab = [np.abs(L[k]).astype(np.float64) for k in range(3)]
        Dab = [np.abs(D[k]).astype(np.float64) for k in range(3)]
        eD = [derivative_error_units(Lab[k], Dab[k], deg) for k in range(3)]
        Nf = (Nd[idx[0]] * Nd[idx[1]] * Nd[idx[2]]).astype(np.float64)
        ca = np.abs(co)
        f[i] = (co.astype(LD) * (L[0] * Nd)[idx[0]] * (L[1] * Nd)[idx[1]] * (L[2] * Nd)[idx[2]]).sum()
        s = LD(float(2 << dep))
        dgu = np.zeros(3)
        for k in range(3):
            o1, o2 = (k + 1) % 3, (k + 2) % 3
            t = co.astype(LD) * (D[k] * Nd)[idx[k]] * (L[o1] * Nd)[idx[o1]] * (L[o2] * Nd)[idx[o2]]
            cs = np.cumsum(t)
            run = float(np.abs(cs[1:]).astype(np.float64).sum())
            dk, l1, l2 = Dab[k][idx[k]], Lab[o1][idx[o1]], Lab[o2][idx[o2]]
            per = eD[k][idx[k]] * l1 * l2 + idx[o1] ** 2 * dk * l2 + idx[o2] ** 2 * dk * l1 + K_G * dk * l1 * l2
            dgu[k] = R.U * ((ca * Nf * per).sum() + run)
            gu[i, k] = cs[-1]
            g[i, k] = cs[-1] * s * LD(inv[k])
        dg = dgu * float(2 << dep) * inv + 2 * R.U * np.abs(g[i]).astype(np.float64)
        gb[i] = dg * R.SLACK
        nrm = np.sqrt(_sum3(g[i, 0] ** 2, g[i, 1] ** 2, g[i, 2] ** 2, left))
        if nrm > 0:
            gn[i] = g[i] / nrm
            gnb[i] = (np.sqrt((dg ** 2).sum()) / float(nrm) + 3.5 * R.U) * R.SLACK
        else:
            gn[i] = g[i]
            gnb[i] = np.inf
    return {"f": f, "g": g, "g_bound": gb, "n": gn, "n_bound": gnb, "gu": gu, "leaf": leaf}


def _sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


def excess(got, ref, unit=False):
    """max |got - reference| / bound over rows and components (unit: against the normalised rows)."""
    want, bound = (ref["n"], ref["n_bound"]) if unit else (ref["g"], ref["g_bound"])
    d = np.abs(np.asarray(got, np.float64).astype(LD) - want).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))
    return float(r.max())


def shortcut_unnormalised(block, points):
    """The reference's FApproxWithGradient shortcut (Octree.cpp:904-985) BEFORE its normalize(), in long double: per axis k the central
    difference of sum_r c_r LN_{idx[r][k]}(x_k +- 1e-4) -- a unit-space quantity that lacks the other two axes' factors -> [n, 3]."""
    blk = block if isinstance(block, R.Block) else R.Block(block)
    q = blk.to_unit(points)
    leaf = blk.descend(q)
    out = np.zeros((len(q), 3), LD)
    for i in range(len(q)):
        n = leaf[i]
        deg, dep = int(blk.degree[n]), int(blk.depth[n])
        cen = ((blk.bmin[n] + blk.bmax[n]) / np.float32(2.0)).astype(np.float64)
        x = (q[i] - cen) * float(2 << dep)
        nc = int(R.COUNT[deg])
        co = blk.coeffs[blk.start[n]:blk.start[n] + nc].astype(LD)
        Nd = R.NL[:deg + 1, dep].astype(LD)
        for k in range(3):
            bk = R.BIDX[:nc, k]
            pm = [(co * (R.legendre_ld(np.array([xe]), deg)[:, 0] * Nd)[bk]).sum() for xe in (x[k] + R.H_GRAD, x[k] - R.H_GRAD)]
            out[i, k] = (pm[0] - pm[1]) / LD(2 * R.H_GRAD)
    return out


def lower_neighbour_leaves(block, points, axis):
    """For points lying ON a cell face across `axis` (where Query takes the upper cell): the leaf on the other side of the face."""
    blk = block if isinstance(block, R.Block) else R.Block(block)
    q = blk.to_unit(points).copy()
    q[:, axis] = np.nextafter(q[:, axis], -np.inf)
    return blk.descend(q)
