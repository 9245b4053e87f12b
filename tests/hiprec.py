"""An extended-precision reference for the per-cell fit (Octree::FitPolynomial, Octree.cpp:1007-1069) and for Query
(Octree::FApprox / FApproxWithGradient, Octree.cpp:662-702, 859-985), independent of the oracle and of the product.

It reads the reference's numbers only from tests/golden/ref_tables.npz and uses them exactly as they are (coeff_count[6] == 83,
rows in basis_index order).  Every quantity the reference's code forms in float32 or float64 *before* the arithmetic under test --
the cell's centre and scale, the sample positions, the query point's unit coordinates, the gradient's offset points -- is
reproduced here bit for bit in numpy; everything after it is computed in np.longdouble (64-bit mantissa).  Each kernel result is
then checked against a worst-case bound derived below from the order of its operations.  No constant was chosen by looking at a
kernel's output.

Notation: u = 2^-53 (unit roundoff of float64).  fl(a op b) = (a op b)(1 + d), |d| <= u.  All bounds are first order; the neglected
terms are products of two relative errors each below (n + 200) u < 2e-11, so every bound is multiplied by SLACK = 1 + 1e-6.

1. Fields (csrc/field_eval.hpp:48-84; hp_oracle.c prim_eval).  eF(x) below is |F_f64(x) - F(x)| / u.
   sphere  d_a = fl(x_a - c_a)                                   rel u each
           fl(d_a^2), two additions of non-negative terms         sum: rel 3u + 2u = 5u
           sqrt (correctly rounded)                              rel 5u/2 + u = 3.5u on rho = |x - c|
           fl(rho - r)                                           + u (rho + r)           => eF <= 4.5 (rho + r)
   box     e_a = |x_a - c_a| rel u; q_a = fl(e_a - h_a)           |dq_a| <= u (2 e_a + h_a)
           outside = norm3(max(q, 0)): 1-Lipschitz in q, + 3.5u |q|;  inside = min(max q_a, 0): + max |dq_a|;  fl(out + in): + u |.|
           with M = sum_a (e_a + h_a):  2M + 3.5M + 2M + M        => eF <= 8.5 M
   torus   sigma = sqrt(fl(dx^2 + dz^2)): squares 3u, the addition u -> 4u; sqrt halves it, + u  -> rel 3u
           l = fl(s - R): |dl| <= u (4 sigma + R);  fl(l^2 + dy^2): <= u (2|l|(4 sigma + R) + 2 l^2 + 4 dy^2)
           tau = sqrt(.): <= that / (2 tau) + u tau <= u (4 sigma + R + 4 tau);  fl(tau - r): + u (tau + r)
                                                                 => eF <= 5 (sigma + tau + R + r)
   plane   fl(fl(p0 x) + fl(fl(p1 y) + fl(p2 z))) + p3: four roundings reach each term at most
                                                                 => eF <= 4 (|p0 x| + |p1 y| + |p2 z| + |p3|)
   CSG     min / max / negation are exact and |min(a + alpha, b + beta) - min(a, b)| <= max(|alpha|, |beta|): eF = max of the operands'.
   The reduction order (hpsdf_set_reduction_order) only permutes the additions counted above; the bounds hold for both orders.
   Data (DataField: a mesh, csrc/field_glue.hpp fieldEvalWorld, hp_oracle.c ora_field_eval ORA_FIELD_MESH; a sample buffer).  The
           field IS a table of float64 numbers, one per sample position: there is no real-valued F behind it that the float64
           value approximates.  For a mesh the number at position X (float64, reproduced bit for bit, section 2) is
               (double) SignedDistanceAtPt((float) X_x, (float) X_y, (float) X_z).
           The cast rounds to nearest and is reproduced bit for bit (numpy's astype(float32) is the same IEEE conversion); the
           scan is float32 arithmetic that the oracle restates statement by statement and the kernels are pinned to bit for bit
           (tests/test_gpu_parity.py, and the anchor of tests/test_gpu_hiprec_fields.py on the very positions used here), so its
           float32 result is reproduced bit for bit; widening float32 to float64 is exact.  The three steps contribute
           nothing:                                              => eF = 0
           What such a fit checks is everything around the table -- the positions handed to it, their cast, which sample meets
           which weight -- and the fit's own arithmetic; not whether the scan is the true distance (DESIGN.md section 2 says why
           exact geometry is no reference for it).
   Tree CSG (CsgField; applyCsg, Octree.cpp:355-400; ora_field_eval ORA_FIELD_TREE_CSG).  With o = FApprox(old tree, X) and
           v = the inner field at X:  union min(o, v), intersect max(o, v), subtract max(-o, v) -- the reference negates the OLD
           tree, as o * -1.0.  Negation and o * -1.0 are exact (a sign flip), min and max are exact, so the argument is the one for
           analytic CSG above: |min(o + alpha, v + beta) - min(o, v)| <= max(|alpha|, |beta|), likewise for max.  The old tree's
           value is section 3's: the descent and the unit coordinates are float64 operations reproduced bit for bit (a point ON a
           face of an old leaf -- the centre node of every odd rule lies on one when the old leaves are deeper than the cell --
           goes to the upper child, >= at :681-683, and Block.descend does the same), the series in long double with its bound
           f_bound.  So alpha <= f_bound and               => eF = max(f_bound / u, eF of the inner field).

2. A fit row r = (a, b, c) of degree p at depth d (Octree.cpp:1028-1056):
       c_r = sum_s t_s,   t_s = L_a(x_i) N_a L_b(x_j) N_b L_c(x_k) N_c * S w_i w_j w_k F(X_s),   n = (4p + 1)^3 samples,
   N_a = normalised_lengths[a][d], S = scale_x scale_y scale_z, (x_q, w_q) the Gauss-Legendre rule of order 4p + 1 (sum_to_n[4p]).
   Per-term error sources, in every fit mode:
   (i)   L_a by the three-term recurrence L_j = rec[j][0] x L_{j-1} - rec[j][1] L_{j-2} in float64: |dL_j| <= j^2 u on [-1, 1]
         (the absolute model; tests/test_hiprec_cpu.py checks it on every node of every rule the fits use).  Its contribution
         to row r is u N S sum_s |w_i w_j w_k F_s| (a^2 |L_b L_c| + b^2 |L_a L_c| + c^2 |L_a L_b|) =: u R_r.
   (ii)  at most K_MUL = 12 multiplicative roundings on each term.  The exact kernel (fit_kernels.hpp, as hp_oracle.c:420-441):
         Lp: 5 (the first *= of 1.0 is exact), S = prod3(scale): 2, wprod: 2, S * wprod: 1, * F: 1, Lp * FaabSample: 1 -> 12.
         The split kernel (fit_low.hip:65-143): A = w P: 1 per axis (3), the three contractions are fused multiply-adds (their
         products exact), then ((S N_a)(N_b N_c)) s: 4, plus S: 2 -> 9.  The matrix-core kernels (fit_mfma.hip) form the same
         factors with no more roundings.  So u K_MUL S_r with S_r = sum_s |t_s|.
   (iii) the summation of the n terms in ANY order or grouping (sequential, per-thread partial sums, the sum-factorised stages,
         an MFMA accumulation tree): each term passes through at most n - 1 roundings of sums whose magnitude is at most
         sum |t_s|, so u (n - 1) S_r.
   (iv)  the field: u E_r, E_r = N S sum_s |L_a L_b L_c w_i w_j w_k| eF(X_s).
   Sample positions are reproduced bit for bit (the product builds with -ffp-contract=off), so they contribute nothing.
       |c_r - c*_r| <= u ((n - 1 + K_MUL) S_r + R_r + E_r) * SLACK.
   One bound for all summation orders: it serves FIT_EXACT, FIT_SPLIT (either lower-row kernel) and FIT_FAST alike.
   The error e = sum over rows of top degree of c_r^2 (:1062-1069), m such rows: with d_r the row bounds,
       |e - e*| <= sum (2 |c*_r| d_r + d_r^2) + u (m + 1) sum (|c*_r| + d_r)^2      (one rounding per square, m - 1 additions).

3. Query (FApprox, Octree.cpp:859-901; hp_oracle.c ora_fapprox).  The descent and the unit coordinates
   x = (pt - centre_f32) * 2^(d+1) are float64 operations reproduced bit for bit; |x| <= 1 inside the leaf.
       f = sum_i c_i P_i,  P_i = LN_a(x) LN_b(y) LN_c(z),  LN_j = fl(L_j N_j)
   per term: the recurrence as (i), 3 roundings of LN, 2 of the product, 1 of c_i P_i -> K_Q = 6; the m terms are added in
   the loop's fixed order (the kernels are pinned to it bit for bit by tests/test_gpu_parity.py), so the summation contributes
   u sum_{i >= 1} |s_i| with s_i the exact partial sums (the first addition, to 0.0, is exact):
       |f - f*| <= u (sum_i |c_i| N (a^2 |L_b L_c| + b^2 |L_a L_c| + c^2 |L_a L_b| + K_Q |L_a L_b L_c|) + sum_{i>=1} |s_i|) SLACK.
   Gradient (FApproxWithGradient, :904-985): per axis k, p = sum_i c_i LN_{b_ik}(fl(x_k + h)), m likewise at fl(x_k - h),
   h = 1e-4; each sum has the bound above with 2 roundings per term (LN, c_i LN) and the recurrence at |x| <= 1 + h (the same
   model, checked there too).  g_k = fl(fl(p - m) / 2h) (2h exact):  |dg_k| <= (dp + dm + u |p - m|) / 2h + u |g_k|  -- the
   1/(2h) amplification.  normalize(): the map g -> g/|g| has Jacobian norm 1/|g|, and z = sum3(g^2) (3u), sqrt (2.5u) and the
   division (3.5u) add 3.5u per component:   |v_k - v*_k| <= |dg|_2 / |g*| + 3.5u.
"""
import os

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double (64-bit mantissa)"

U = 2.0 ** -53
SLACK = 1.0 + 1e-6
K_MUL = 12
K_Q = 6
H_GRAD = 1e-4
PRIM_SPHERE, PRIM_BOX, PRIM_TORUS_Y, PRIM_PLANE = 0, 1, 2, 3
OP_UNION, OP_INTERSECT, OP_SUBTRACT = 0, 1, 2
LEAF = 0xFFFFFFFFFFFFFFFF
INTERIOR = 13

_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tables.npz"))
ROOTS = _Z["roots"]
WEIGHTS = _Z["weights"]
NL = _Z["normalised_lengths"]
REC = _Z["recurrence"]
COUNT = _Z["coeff_count"].astype(np.int64)
BIDX = _Z["basis_index"].astype(np.int64)
SUMTON = _Z["sum_to_n"].astype(np.int64)


def rule(n):
    """Gauss-Legendre rule of order n: rule n starts at n(n - 1)/2 = sum_to_n[n - 1] (Legendre.h; Octree.cpp:1016-1017; the
    table of sums stops at 49, the rules at 64)."""
    s = n * (n - 1) // 2
    return ROOTS[s:s + n], WEIGHTS[s:s + n]


def legendre_ld(x, p, rec=REC):
    """L_0..L_p at x (float64 array) by Octree::LpX's recurrence (:988-1004), in long double -> [p + 1, len(x)]."""
    x = np.asarray(x, np.float64).astype(LD)
    out = np.empty((p + 1,) + x.shape, LD)
    m2, m1 = np.zeros_like(x), np.ones_like(x)
    out[0] = 1
    for j in range(1, p + 1):
        li = LD(rec[j][0]) * x * m1 - LD(rec[j][1]) * m2
        m2, m1 = m1, li
        out[j] = li
    return out


def legendre_f64(x, p, rec=REC):
    """The same recurrence in float64 without contraction (the kernels build with -ffp-contract=off)."""
    x = np.asarray(x, np.float64)
    out = np.empty((p + 1,) + x.shape)
    m2, m1 = np.zeros_like(x), np.ones_like(x)
    out[0] = 1.0
    for j in range(1, p + 1):
        li = rec[j][0] * x * m1 - rec[j][1] * m2
        m2, m1 = m1, li
        out[j] = li
    return out


# ---------------------------------------------------------------------------------------------------------------- fields
def _sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


class DataField:
    """A field that is data (section 1): values(points_f64[n, 3]) -> float64[n], the numbers the fit is handed at the reproduced
    sample positions, taken as exact (eF = 0)."""

    def __init__(self, values):
        self.values = values


def mesh_field(mesh, mutant=None):
    """A mesh as data.  mesh: an object with signed_distance(points_f32[n, 3]) -> (float32[n], ...) -- the oracle's O(n) scan
    (O.MeshField), never a traversal or a fit of the product.  The positions are cast to float32 (round to nearest, as (float) x
    does), the scan's float32 value is widened.  mutant "ulp": the positions one float32 ulp up before the cast."""
    assert mutant in (None, "ulp"), mutant

    def values(pts):
        pts = np.asarray(pts, np.float64)
        if mutant == "ulp":
            pts = pts + np.spacing(pts.astype(np.float32)).astype(np.float64)
        return mesh.signed_distance(np.ascontiguousarray(pts.astype(np.float32)))[0].astype(np.float64)
    return DataField(values)


class CsgField:
    """(old_block, op, inner): the tree-CSG wrapper of Octree.cpp:355-400 around an inner field (a spec list or a DataField).
    mutant (tests/test_hiprec_fields_cpu.py): "subtract_swapped" max(old, -F), "union_max", "tree_f32" the old tree evaluated at
    the float32-cast point, "tie_low" a point on an old leaf's face sent to the lower child."""

    def __init__(self, old_block, op, inner, mutant=None):
        self.block = old_block if isinstance(old_block, Block) else Block(old_block)
        self.op, self.inner, self.mutant = op, inner, mutant


def _points(X, Y, Z):
    shape = np.broadcast(X, Y, Z).shape
    return np.stack([np.broadcast_to(np.asarray(v, np.float64), shape).ravel() for v in (X, Y, Z)], 1), shape


def field_eval(spec, X, Y, Z, left=False):
    """A field at float64 points -> (value in long double, eF / u).  spec: an analytic field [(kind, op, params)] (as
    Field.analytic), a DataField or a CsgField."""
    if isinstance(spec, DataField):
        pts, shape = _points(X, Y, Z)
        v = np.asarray(spec.values(pts), np.float64)
        return v.astype(LD).reshape(shape), np.zeros(shape)
    if isinstance(spec, CsgField):
        pts, shape = _points(X, Y, Z)
        v, e = field_eval(spec.inner, X, Y, Z, left)
        v, e = np.broadcast_to(v, shape), np.broadcast_to(e, shape)
        tp = pts.astype(np.float32).astype(np.float64) if spec.mutant == "tree_f32" else pts
        old = fapprox_batch(spec.block, tp, tie_low=spec.mutant == "tie_low")
        o = old["f"].reshape(shape)
        if spec.op == OP_UNION:
            out = np.maximum(o, v) if spec.mutant == "union_max" else np.minimum(o, v)
        elif spec.op == OP_SUBTRACT:
            out = np.maximum(o, -v) if spec.mutant == "subtract_swapped" else np.maximum(-o, v)
        elif spec.op == OP_INTERSECT:
            out = np.maximum(o, v)
        else:
            raise ValueError(spec.op)
        return out, np.maximum(e, (old["f_bound"] / U).reshape(shape))
    x, y, z = (np.asarray(v, np.float64).astype(LD) for v in (X, Y, Z))
    acc = acc_e = None
    for kind, op, p in spec:
        p = [LD(float(v)) for v in p]
        if kind == PRIM_SPHERE:
            dx, dy, dz = x - p[0], y - p[1], z - p[2]
            rho = np.sqrt(_sum3(dx * dx, dy * dy, dz * dz, left))
            v, e = rho - p[3], 4.5 * (rho + abs(p[3]))
        elif kind == PRIM_BOX:
            ex, ey, ez = abs(x - p[0]), abs(y - p[1]), abs(z - p[2])
            qx, qy, qz = ex - p[3], ey - p[4], ez - p[5]
            zero = LD(0)
            out = np.sqrt(_sum3(np.maximum(qx, zero) ** 2, np.maximum(qy, zero) ** 2, np.maximum(qz, zero) ** 2, left))
            v = out + np.minimum(np.maximum(qx, np.maximum(qy, qz)), zero)
            e = 8.5 * (ex + ey + ez + abs(p[3]) + abs(p[4]) + abs(p[5]))
        elif kind == PRIM_TORUS_Y:
            dx, dy, dz = x - p[0], y - p[1], z - p[2]
            sig = np.sqrt(dx * dx + dz * dz)
            l = sig - p[3]
            tau = np.sqrt(l * l + dy * dy)
            v, e = tau - p[4], 5.0 * (sig + tau + abs(p[3]) + abs(p[4]))
        elif kind == PRIM_PLANE:
            a0, a1, a2 = p[0] * x, p[1] * y, p[2] * z
            v, e = (a0 + (a1 + a2)) + p[3], 4.0 * (abs(a0) + abs(a1) + abs(a2) + abs(p[3]))
        else:
            raise ValueError(kind)
        if acc is None:
            acc, acc_e = v, e
        else:
            acc = np.minimum(acc, v) if op == OP_UNION else np.maximum(acc, v) if op == OP_INTERSECT else np.maximum(acc, -v)
            acc_e = np.maximum(acc_e, e)
    return acc, np.asarray(acc_e, np.float64)


# ---------------------------------------------------------------------------------------------------------------- fits
def lattice_cells(depth, n):
    """The first n cells of the depth-`depth` lattice, x fastest, wrapping after side^3 (hpsdf_fit_cells, bench_fit.cpp) -> f32 bmin, bmax."""
    side = 1 << depth
    h = np.float32(1.0) / np.float32(side)
    i = np.arange(n) % (side ** 3)
    idx = np.stack([i % side, (i // side) % side, i // (side * side)], 1)
    bmin = np.float32(-0.5) + idx.astype(np.float32) * h
    return bmin.astype(np.float32), (bmin + h).astype(np.float32)


def _contract(mx, my, mz, t):
    """R[C, a, b, c] = sum_ijk mx[a, i] my[b, j] mz[c, k] t[C, i, j, k] (three one-axis contractions)."""
    g1 = np.einsum("ai,Cijk->Cajk", mx, t)
    g2 = np.einsum("bj,Cajk->Cabk", my, g1)
    return np.einsum("ck,Cabk->Cabc", mz, g2)


def sample_axes(root_min, root_max, bmin, bmax, nq):
    """The world coordinates of a fit's samples, per axis, as the reference and the kernels form them in float64 -> ([3] arrays
    [C, nq], the cells' float64 half-extents [C, 3]).  Sample (i, j, k) of cell C lies at (wx[0][C, i], wx[1][C, j], wx[2][C, k])."""
    bmin = np.atleast_2d(np.asarray(bmin, np.float32))
    bmax = np.atleast_2d(np.asarray(bmax, np.float32))
    x, _ = rule(nq)
    # :1020-1022, the product's FitTask: sizes() and center() in float32, then widened
    scale = (bmax - bmin).astype(np.float64) * 0.5
    centre = ((bmin + bmax) / np.float32(2.0)).astype(np.float64)
    rmin, rmax = np.asarray(root_min, np.float32), np.asarray(root_max, np.float32)
    rb = (rmax - rmin).astype(np.float64)
    rc = ((rmin + rmax) / np.float32(2.0)).astype(np.float64)
    # :1039 and :327 (fit_kernels.hpp: w = u * bounds + centre): float64, unfused
    return [(x[None, :] * scale[:, a:a + 1] + centre[:, a:a + 1]) * rb[a] + rc[a] for a in range(3)], scale


def fit_reference(spec, root_min, root_max, bmin, bmax, degree, depth, left=False, *, order=None, nl_depth=None,
                  samples_f32=False, zero_sample=None):
    """Octree::FitPolynomial of `degree` at `depth` for cells bmin, bmax ([C, 3] float32, root-normalised) under the root
    [root_min, root_max] -> dict(c=[C, ncoef] long double, bound=[C, ncoef], e=[C] long double, e_bound=[C]).  spec: whatever
    field_eval takes -- an analytic spec, a DataField or a CsgField.
    The keyword arguments build mutants (tests/test_hiprec_cpu.py): another Gauss order, NormalisedLengths of another depth,
    samples rounded to float32, one sample's weight zeroed (its (i, j, k))."""
    bmin = np.atleast_2d(np.asarray(bmin, np.float32))
    bmax = np.atleast_2d(np.asarray(bmax, np.float32))
    C = len(bmin)
    p = degree
    nq = 4 * p + 1 if order is None else order
    x, w = rule(nq)
    wx, scale = sample_axes(root_min, root_max, bmin, bmax, nq)
    X = np.broadcast_to(wx[0][:, :, None, None], (C, nq, nq, nq))
    Y = np.broadcast_to(wx[1][:, None, :, None], (C, nq, nq, nq))
    Zc = np.broadcast_to(wx[2][:, None, None, :], (C, nq, nq, nq))
    F, eF = field_eval(spec, X, Y, Zc, left)
    if samples_f32:
        F = F.astype(np.float64).astype(np.float32).astype(LD)
    if zero_sample is not None:
        F = F.copy()
        F[:, zero_sample[0], zero_sample[1], zero_sample[2]] = 0
    L = legendre_ld(x, p)                                   # [p + 1, nq]
    A = LD(1) * w.astype(LD)[None, :] * L                   # w_q L_a(x_q)
    Aabs = np.abs(A).astype(np.float64)
    W2 = (np.arange(p + 1, dtype=np.float64) ** 2)[:, None] * np.abs(w)[None, :]
    Fabs = np.abs(F).astype(np.float64)
    S = scale[:, 0].astype(LD) * scale[:, 1].astype(LD) * scale[:, 2].astype(LD)
    R = _contract(A, A, A, F)
    Rs = _contract(Aabs, Aabs, Aabs, Fabs)
    Rr = _contract(W2, Aabs, Aabs, Fabs) + _contract(Aabs, W2, Aabs, Fabs) + _contract(Aabs, Aabs, W2, Fabs)
    Re = _contract(Aabs, Aabs, Aabs, eF)
    nc = int(COUNT[p])
    a, b, c = BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]
    dn = depth if nl_depth is None else nl_depth
    N = NL[a, dn].astype(LD) * NL[b, dn].astype(LD) * NL[c, dn].astype(LD)
    cs = S[:, None] * N[None, :] * R[:, a, b, c]
    scaleN = (S[:, None] * N[None, :]).astype(np.float64)
    n = (4 * p + 1) ** 3
    bound = U * scaleN * ((n - 1 + K_MUL) * Rs[:, a, b, c] + Rr[:, a, b, c] + Re[:, a, b, c]) * SLACK
    top = (a + b + c) == p
    e = (cs[:, top] ** 2).sum(1)
    ca, d = np.abs(cs[:, top]).astype(np.float64), bound[:, top]
    m = int(top.sum())
    e_bound = ((2 * ca * d + d * d).sum(1) + U * (m + 1) * ((ca + d) ** 2).sum(1)) * SLACK
    return {"c": cs, "bound": bound, "e": e, "e_bound": e_bound}


def fit_ratio(ref, coeffs, errs=None):
    """max |kernel - reference| / bound over coefficients (and errors, if given) -> (coeff ratio, error ratio)."""
    dc = np.abs(np.asarray(coeffs, np.float64).astype(LD) - ref["c"]).astype(np.float64)
    rc = float((dc / ref["bound"]).max())
    re = 0.0
    if errs is not None:
        de = np.abs(np.asarray(errs, np.float64).astype(LD) - ref["e"]).astype(np.float64)
        re = float((de / ref["e_bound"]).max())
    return rc, re


# ---------------------------------------------------------------------------------------------------------------- query
class Block:
    """A serialised MemoryBlock (Include/HP/MemoryBlock.h): coefficients, 56-byte nodes, 80-byte config."""

    def __init__(self, blk):
        blk = bytes(blk)
        nc = int(np.frombuffer(blk, np.uint64, 1, 0)[0])
        self.coeffs = np.frombuffer(blk, np.float64, nc, 8).copy()
        off = 8 + 8 * nc
        nn = int(np.frombuffer(blk, np.uint64, 1, off)[0])
        raw = np.frombuffer(blk, np.uint8, 56 * nn, off + 8).reshape(nn, 56)
        self.child = raw[:, 0:8].copy().view(np.uint64)[:, 0]
        self.bmin = raw[:, 8:20].copy().view(np.float32)
        self.bmax = raw[:, 20:32].copy().view(np.float32)
        self.start = raw[:, 32:40].copy().view(np.uint64)[:, 0].astype(np.int64)
        self.degree = raw[:, 40].astype(np.int64)
        self.depth = raw[:, 48].astype(np.int64)
        cfg = np.frombuffer(blk, np.uint8, 80, off + 8 + 56 * nn)
        self.root_min = cfg[56:68].copy().view(np.float32)
        self.root_max = cfg[68:80].copy().view(np.float32)

    def leaves(self):
        return np.nonzero(self.degree != INTERIOR)[0]

    def to_unit(self, pts):
        """Octree.cpp:665 (hp_oracle.c set_root_vectors): float32 centre, float32 reciprocal of the float32 size."""
        rc = ((self.root_min + self.root_max) / np.float32(2.0)).astype(np.float64)
        inv = (np.float32(1.0) / (self.root_max - self.root_min)).astype(np.float64)
        return (np.asarray(pts, np.float64) - rc) * inv

    def from_unit(self, q):
        rc = ((self.root_min + self.root_max) / np.float32(2.0)).astype(np.float64)
        inv = (np.float32(1.0) / (self.root_max - self.root_min)).astype(np.float64)
        return np.asarray(q, np.float64) / inv + rc

    def descend(self, q, tie_low=False):
        """Octree.cpp:668-702 on root-normalised points (all inside the root) -> leaf index per point.  tie_low: the mutant that
        sends a point on a face to the lower child (> for >=)."""
        cur = np.zeros(len(q), np.int64)
        out = np.full(len(q), -1, np.int64)
        live = np.arange(len(q))
        while len(live):
            n = cur[live]
            half = (self.bmax[n, 0] - self.bmin[n, 0]) * np.float32(0.5)       # :679 the x extent on every axis
            idx = np.zeros(len(live), np.int64)
            for a in range(3):
                mid = (self.bmin[n, a] + half).astype(np.float64)
                idx += (q[live, a] > mid if tie_low else q[live, a] >= mid).astype(np.int64) << a
            ch = self.child[n].astype(np.int64) + idx
            leaf = self.degree[ch] != INTERIOR
            out[live[leaf]] = ch[leaf]
            cur[live] = ch
            live = live[~leaf]
        return out


def _series(coeffs, Lf, deg):
    """sum_i c_i Lf_a(x) Lf_b(y) Lf_c(z) with Lf = L N ([3][p + 1] long double), and the bound's two sums."""
    nc = int(COUNT[deg])
    a, b, c = BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]
    t = coeffs.astype(LD) * Lf[0][a] * Lf[1][b] * Lf[2][c]
    s = np.cumsum(t)
    return s[-1], t, a, b, c, float(np.abs(s[1:]).astype(np.float64).sum())


def fapprox_reference(block, points, gradient=False, rec=REC):
    """Query (FApprox) of a MemoryBlock at world points inside its leaves -> dict(f, f_bound[, g, g_bound]); long double values."""
    blk = block if isinstance(block, Block) else Block(block)
    q = blk.to_unit(points)
    leaf = blk.descend(q)
    npt = len(q)
    f, fb = np.empty(npt, LD), np.empty(npt)
    g, gb = np.zeros((npt, 3), LD), np.zeros((npt, 3))
    for i in range(npt):
        n = leaf[i]
        deg, dep = int(blk.degree[n]), int(blk.depth[n])
        cen = ((blk.bmin[n] + blk.bmax[n]) / np.float32(2.0)).astype(np.float64)
        x = (q[i] - cen) * float(2 << dep)                   # :862, float64
        co = blk.coeffs[blk.start[n]:blk.start[n] + int(COUNT[deg])]
        Nd = NL[:deg + 1, dep].astype(LD)
        L = [legendre_ld(np.array([x[k]]), deg, rec)[:, 0] for k in range(3)]
        val, t, a, b, c, run = _series(co, [L[k] * Nd for k in range(3)], deg)
        Lab = [np.abs(L[k]).astype(np.float64) for k in range(3)]
        Nf = (Nd[a] * Nd[b] * Nd[c]).astype(np.float64)
        ca = np.abs(co)
        rec_t = (a ** 2 * Lab[1][b] * Lab[2][c] + b ** 2 * Lab[0][a] * Lab[2][c] + c ** 2 * Lab[0][a] * Lab[1][b])
        f[i] = val
        fb[i] = U * ((ca * Nf * (rec_t + K_Q * Lab[0][a] * Lab[1][b] * Lab[2][c])).sum() + run) * SLACK
        if gradient:
            dg = np.zeros(3)
            for k in range(3):
                bk = BIDX[:int(COUNT[deg]), k]
                pm, pb = [], []
                for xe in (x[k] + H_GRAD, x[k] - H_GRAD):               # :941, :945: the offset points in float64
                    Le = legendre_ld(np.array([xe]), deg, rec)[:, 0]
                    te = co.astype(LD) * (Le * Nd)[bk]
                    se = np.cumsum(te)
                    pm.append(se[-1])
                    le = np.abs(Le).astype(np.float64)
                    pb.append(U * ((ca * Nd[bk].astype(np.float64) * (bk ** 2 + 2 * le[bk])).sum()
                                   + float(np.abs(se[1:]).astype(np.float64).sum())))
                g[i, k] = (pm[0] - pm[1]) / LD(2 * H_GRAD)
                dg[k] = (pb[0] + pb[1] + U * float(abs(pm[0] - pm[1]))) / (2 * H_GRAD) + U * float(abs(g[i, k]))
            nrm = np.sqrt((g[i] ** 2).sum())
            if nrm > 0:
                g[i] = g[i] / nrm
                gb[i] = (np.sqrt((dg ** 2).sum()) / float(nrm) + 3.5 * U) * SLACK
            else:
                gb[i] = np.inf
    out = {"f": f, "f_bound": fb, "leaf": leaf}
    if gradient:
        out["g"], out["g_bound"] = g, gb
    return out


def fapprox_batch(block, points, tie_low=False):
    """fapprox_reference's value and bound (no gradient) for many points, leaves of one (degree, depth) at a time: the same
    long-double operations in the same order, vectorised over the points -> dict(f, f_bound, leaf)."""
    blk = block if isinstance(block, Block) else Block(block)
    q = blk.to_unit(points)
    leaf = blk.descend(q, tie_low)
    f, fb = np.empty(len(q), LD), np.empty(len(q))
    key = blk.degree[leaf] * 16 + blk.depth[leaf]
    for k in np.unique(key):
        deg, dep = int(k) // 16, int(k) % 16
        nc = int(COUNT[deg])
        a, b, c = BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]
        Nd = NL[:deg + 1, dep].astype(LD)
        Nf = (Nd[a] * Nd[b] * Nd[c]).astype(np.float64)
        sel = np.nonzero(key == k)[0]
        step = max(1, 2 ** 19 // nc)
        for i in range(0, len(sel), step):
            s = sel[i:i + step]
            n = leaf[s]
            cen = ((blk.bmin[n] + blk.bmax[n]) / np.float32(2.0)).astype(np.float64)
            x = (q[s] - cen) * float(2 << dep)                   # :862, float64
            co = blk.coeffs[blk.start[n][:, None] + np.arange(nc)[None, :]]
            L = [legendre_ld(x[:, j], deg) for j in range(3)]     # [deg + 1, m] each
            Lf = [L[j] * Nd[:, None] for j in range(3)]
            t = co.astype(LD) * Lf[0][a].T * Lf[1][b].T * Lf[2][c].T
            cs = np.cumsum(t, axis=1)
            run = np.abs(cs[:, 1:]).astype(np.float64).sum(1)
            Lab = [np.abs(L[j]).astype(np.float64) for j in range(3)]
            la, lb, lc = Lab[0][a].T, Lab[1][b].T, Lab[2][c].T
            rec_t = a ** 2 * lb * lc + b ** 2 * la * lc + c ** 2 * la * lb
            f[s] = cs[:, -1]
            fb[s] = U * ((np.abs(co) * Nf * (rec_t + K_Q * la * lb * lc)).sum(1) + run) * SLACK
    return {"f": f, "f_bound": fb, "leaf": leaf}


def points_in_leaves(block, rng, n, margin=2.0 ** -20):
    """n world points, each strictly inside a random leaf: at least `margin` of the cell from any face."""
    blk = block if isinstance(block, Block) else Block(block)
    lv = blk.leaves()
    pick = lv[rng.integers(0, len(lv), n)]
    lo = blk.bmin[pick].astype(np.float64)
    ext = (blk.bmax[pick] - blk.bmin[pick]).astype(np.float64)
    q = lo + ext * (margin + (1 - 2 * margin) * rng.random((n, 3)))
    return blk.from_unit(q)


# ---------------------------------------------------------------------------------------------------------------- fields at the lattice's corner
def corner_fields(root_min, root_max, depth):
    """Analytic fields whose features lie in the first cells of the depth-`depth` lattice (the (-,-,-) corner, where
    hpsdf_fit_cells starts): a sphere's surface, a box's corner and edges, the crease of a union of two spheres, a CSG carve
    (intersection and subtraction) and a plane (a polynomial of degree 1: every row above degree 1 is zero to rounding)."""
    rmin, rmax = np.asarray(root_min, np.float64), np.asarray(root_max, np.float64)
    h = 1.0 / (1 << depth)
    bx = (rmax - rmin) * h                       # a cell's extent in world units, per axis

    def at(fx, fy, fz):                          # world point at these fractions of cell 0
        return list(rmin + bx * np.array([fx, fy, fz]))

    r = 0.55 * bx[0]
    big = list((rmax - rmin) * 0.4)
    bmn = np.array(at(0.3, 0.35, 0.4))
    return {
        "sphere": [(PRIM_SPHERE, OP_UNION, at(0.2, 0.3, 0.25) + [r])],
        "box": [(PRIM_BOX, OP_UNION, list(bmn + np.array(big)) + big)],
        "crease": [(PRIM_SPHERE, OP_UNION, at(0.1, 0.45, 0.5) + [r]), (PRIM_SPHERE, OP_UNION, at(0.9, 0.55, 0.5) + [r])],
        "carve": [(PRIM_BOX, OP_UNION, list(bmn + np.array(big)) + big), (PRIM_SPHERE, OP_INTERSECT, at(0.5, 0.5, 0.5) + [1.5 * r]),
                  (PRIM_TORUS_Y, OP_SUBTRACT, at(0.6, 0.5, 0.6) + [0.3 * r, 0.1 * r])],
        "plane": [(PRIM_PLANE, OP_UNION, [0.48, -0.6, 0.64, float(-(0.48 * at(.5, .5, .5)[0] - 0.6 * at(.5, .5, .5)[1]
                                                                     + 0.64 * at(.5, .5, .5)[2]))])],
    }
