"""An extended-precision reference for QueryHessian (include/hpsdf.h; csrc/leaf_jet.hpp) on top of hiprec.Block, and a worst-case
bound per Hessian entry derived from the order of the operations, in the manner of hiprec_gradient.py.

What the product forms in float64 before the arithmetic under test -- the root remap (hiprec.Block.to_unit), the descent
(Block.descend) and the leaf's unit coordinates x = (q - centre) * (2 << d) -- is reproduced bit for bit in numpy; everything after
it runs in np.longdouble.  u = 2^-53; bounds are first order and multiplied by hiprec.SLACK.  No constant was chosen by looking at
the implementation's output.

The operation, per leaf (degree p, depth d, coefficients c_i in basis order (a, b, c), N_j = normalised_lengths[j][d]):
    L_j, D_j as hiprec_gradient states them;   E_0 = E_1 = 0, E_j = fl(E_{j-2} + fl((2j-1) D_{j-1}));   EN_j = fl(E_j N_j)
    hu_xx = sum_i fl(c_i fl(fl(EN_a(x) LN_b(y)) LN_c(z)))  in the loop's fixed order from 0.0;  yy, zz with E on the other axes;
    hu_xy = sum_i fl(c_i fl(fl(DN_a(x) DN_b(y)) LN_c(z)));  xz, yz with the two D on the other pairs of axes
    H_kl  = fl(fl(fl(fl(hu_kl 2^(d+1)) 2^(d+1)) inv_k) inv_l),  inv the float64 widening of the tree's float32 reciprocal root sizes

Error sources, |x|, |y|, |z| <= 1 (W_j(t) stands for the factor an entry takes on an axis: L_j, D_j or E_j):
  (i)   the recurrence: |dL_j| <= j^2 u (hiprec section 2 (i)).
  (ii)  |dD_j| <= u eD_j as hiprec_gradient (ii) derives it.
  (ii') the second derivative's accumulation, by the same argument one level up.  E_j is a sum of at most floor(j/2) terms
        (2k+1) D_k, k = j-1, j-3, ... >= 1; each term carries the error of its D_k scaled by (2k+1), one product rounding
        u (2k+1) |D_k|, and each partial sum E_m, m = j, j-2, ... >= 2, one addition rounding u |E_m| (the first addition, to
        E_0 = 0 or E_1 = 0, is exact; it is counted all the same):
            |dE_j| <= u eE_j,   eE_j = sum_{k = j-1, j-3, .. >= 1} (2k+1) (eD_k + |D_k|)  +  sum_{m = j, j-2, .. >= 2} |E_m|,  eE_0 = eE_1 = 0.
  (iii) per term: the three normalised factors one rounding each (3), the two products (2), c_i times the product (1): K_H = 6
        roundings on |c_i| N_a N_b N_c |W_a W_b W_c|; and each factor's own error eW (j^2, eD_j or eE_j) times the other two factors.
  (iv)  the running sum: u sum_{i >= 1} |s_i| with s_i the exact partial sums (the addition to 0.0 is exact).
  So  |dhu| <= u ( sum_i |c_i| N_a N_b N_c ( eW_a |W_b W_c| + eW_b |W_a W_c| + eW_c |W_a W_b| + K_H |W_a W_b W_c| ) + sum_{i>=1} |s_i| ).
  (v)   the world scaling: four products, of which the two by 2^(d+1) are exact:  |dH_kl| <= |dhu_kl| 4^(d+1) inv_k inv_l + 2u |H_kl|.
The curvature is a function of the returned g and H rows alone and is checked bit for bit against a float64 restatement
(tests/test_query_hessian_cpu.py), not against a bound; curvature_ld below is the same formula in long double on the reference's own
g and H, for the sphere check.
"""
import numpy as np

import hiprec as R
import hiprec_gradient as G

LD = R.LD
K_H = 6
ENTRIES = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # xx, yy, zz, xy, xz, yz


def second_derivative_ld(D, p, scale=None):
    """E_0..E_p from D_0..D_p (long double, [p + 1]) by the stated recurrence.  scale: {j: factor on the constant (2j-1)} (mutants)."""
    E = np.zeros(p + 1, LD)
    for j in range(2, p + 1):
        k = LD(2 * j - 1) * (LD(scale[j]) if scale and j in scale else LD(1))
        E[j] = E[j - 2] + k * D[j - 1]
    return E


def second_derivative_error_units(Dabs, Eabs, eD, p):
    """eE_j of (ii'), j = 0..p, from |D_k|, |E_m| (float64) and eD_k."""
    e = np.zeros(p + 1)
    for j in range(2, p + 1):
        e[j] = sum((2 * k + 1) * (eD[k] + Dabs[k]) for k in range(j - 1, 0, -2)) + sum(Eabs[m] for m in range(j, 1, -2))
    return e


def _sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


def curvature_ld(g, H, left=False):
    """(mean, gauss) by the stated formula from rows g [n,3] and H [n,6], in the dtype given (long double for the reference)."""
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    Hxx, Hyy, Hzz, Hxy, Hxz, Hyz = (H[:, k] for k in range(6))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = _sum3(g0 * g0, g1 * g1, g2 * g2, left)
        Hg0 = _sum3(Hxx * g0, Hxy * g1, Hxz * g2, left)
        Hg1 = _sum3(Hxy * g0, Hyy * g1, Hyz * g2, left)
        Hg2 = _sum3(Hxz * g0, Hyz * g1, Hzz * g2, left)
        q = _sum3(g0 * Hg0, g1 * Hg1, g2 * Hg2, left)
        tr = _sum3(Hxx, Hyy, Hzz, left)
        mean = (z * tr - q) / ((2 * z) * np.sqrt(z))
        A00, A11, A22 = Hyy * Hzz - Hyz * Hyz, Hxx * Hzz - Hxz * Hxz, Hxx * Hyy - Hxy * Hxy
        A01, A02, A12 = Hxz * Hyz - Hxy * Hzz, Hxy * Hyz - Hxz * Hyy, Hxy * Hxz - Hxx * Hyz
        Ag0 = _sum3(A00 * g0, A01 * g1, A02 * g2, left)
        Ag1 = _sum3(A01 * g0, A11 * g1, A12 * g2, left)
        Ag2 = _sum3(A02 * g0, A12 * g1, A22 * g2, left)
        k = _sum3(g0 * Ag0, g1 * Ag1, g2 * Ag2, left)
        gauss = k / (z * z)
    ok = z > 0
    nan = np.array(np.nan, mean.dtype)
    return np.stack([np.where(ok, mean, nan), np.where(ok, gauss, nan)], axis=1)


def hessian_reference(block, points, left=False, escale=None, leaf=None, inv_twice=False):
    """QueryHessian of a MemoryBlock at world points inside the root -> dict(f, g [n,3], H [n,6] long double, H_bound [n,6], curv [n,2]
    long double from g and H, leaf).  Mutants: escale {j: factor on E_j's constant}; leaf: evaluate from these leaves instead of the
    descent's; inv_twice: the first axis' reciprocal root size applied twice in place of both axes'."""
    blk = block if isinstance(block, R.Block) else R.Block(block)
    q = blk.to_unit(points)
    leaf = blk.descend(q) if leaf is None else np.asarray(leaf)
    inv = (np.float32(1.0) / (blk.root_max - blk.root_min)).astype(np.float64)
    npt = len(q)
    f = np.empty(npt, LD)
    g = np.zeros((npt, 3), LD)
    H, Hb = np.zeros((npt, 6), LD), np.zeros((npt, 6))
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
        D = [G.derivative_ld(L[k], deg) for k in range(3)]
        E = [second_derivative_ld(D[k], deg, escale) for k in range(3)]
        W = (L, D, E)                                        # W[kind][axis]: kind 0, 1, 2 = the polynomial, its first, its second derivative
        Wab = [[np.abs(W[kind][k]).astype(np.float64) for k in range(3)] for kind in range(3)]
        eD = [G.derivative_error_units(Wab[0][k], Wab[1][k], deg) for k in range(3)]
        eE = [second_derivative_error_units(Wab[1][k], Wab[2][k], eD[k], deg) for k in range(3)]
        eW = ([np.arange(deg + 1, dtype=np.float64) ** 2] * 3, eD, eE)
        Nf = (Nd[idx[0]] * Nd[idx[1]] * Nd[idx[2]]).astype(np.float64)
        ca, cl = np.abs(co), co.astype(LD)
        s = LD(float(2 << dep))
        f[i] = (cl * (L[0] * Nd)[idx[0]] * (L[1] * Nd)[idx[1]] * (L[2] * Nd)[idx[2]]).sum()
        for k in range(3):
            kinds = [1 if ax == k else 0 for ax in range(3)]
            g[i, k] = (cl * (W[kinds[0]][0] * Nd)[idx[0]] * (W[kinds[1]][1] * Nd)[idx[1]] * (W[kinds[2]][2] * Nd)[idx[2]]).sum() * s * LD(inv[k])
        for e, (k, l) in enumerate(ENTRIES):
            kinds = [0, 0, 0]
            kinds[k] += 1
            kinds[l] += 1
            t = cl * (W[kinds[0]][0] * Nd)[idx[0]] * (W[kinds[1]][1] * Nd)[idx[1]] * (W[kinds[2]][2] * Nd)[idx[2]]
            cs = np.cumsum(t)
            run = float(np.abs(cs[1:]).astype(np.float64).sum())
            w = [Wab[kinds[ax]][ax][idx[ax]] for ax in range(3)]
            ew = [eW[kinds[ax]][ax][idx[ax]] for ax in range(3)]
            per = ew[0] * w[1] * w[2] + ew[1] * w[0] * w[2] + ew[2] * w[0] * w[1] + K_H * w[0] * w[1] * w[2]
            dhu = R.U * ((ca * Nf * per).sum() + run)
            ik, il = (inv[k], inv[k]) if inv_twice else (inv[k], inv[l])
            H[i, e] = cs[-1] * s * s * LD(ik) * LD(il)
            Hb[i, e] = (dhu * float(2 << dep) ** 2 * inv[k] * inv[l] + 2 * R.U * abs(float(H[i, e]))) * R.SLACK
    return {"f": f, "g": g, "H": H, "H_bound": Hb, "curv": curvature_ld(g, H, left), "leaf": leaf}


def excess(got, ref):
    """max |got - reference| / bound over rows and the six entries."""
    d = np.abs(np.asarray(got, np.float64).astype(LD) - ref["H"]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(ref["H_bound"] > 0, d / ref["H_bound"], np.where(d > 0, np.inf, 0.0))
    return float(r.max())
