"""An extended-precision reference for the continuity post-process (Octree.cpp:1250-1762): the jump-energy matrix M as exact
face integrals, and the system (M + lambda I) x = lambda c with its true residual -- independent of the oracle and of the product.

It reads the reference's numbers only from tests/golden/ref_tables.npz (through hiprec) and a serialised block (hiprec.Block).
No NodeProc / FaceProc traversal is restated: face pairs come from the leaves' boxes alone.

0. The operation.  A leaf of depth d with box [bmin, bmax] (root-normalised, float32) carries the basis
       phi_i(q) = prod_a N_{i_a}[d] L_{i_a}(x_a),   x = (q - centre) 2^(d+1)   (as Query forms it, Octree.cpp:862),
   orthonormal over the cell.  Two leaves A, B are a pair when their boxes touch in one dimension `dim` (A.bmax == B.bmin, exact
   float32 equality) and overlap with positive area in the other two; S is the overlap.  The pair contributes
       own A   + int_S phi^A_i phi^A_j dA        own B   + int_S phi^B_i phi^B_j dA        cross  - int_S phi^A_i phi^B_j dA (and transposed)
   so that x^T M x = sum over pairs of int_S (f_A - f_B)^2 dA, the integrated squared jump.  Every integrand is a polynomial of degree
   <= 2 max(p_A, p_B) per in-face axis: the Gauss rule of order n = max(p_A, p_B) + 1 (exact to degree 2n - 1) integrates it exactly,
   and the integral factorises into two 1-D quadratures, the face values L(+-1) and the weights.  All of it in np.longdouble.

1. Quantities the product forms in float32 / float64 before the arithmetic under test, reproduced bit for bit (prepareNumericFace,
   Octree.cpp:1264-1290): the shared face's extent (float32 max / min / subtraction, widened, * 0.5) and scale12; invDist =
   1 / 2^depthDiff; invT[m] = (double)(cs - cl) / ((double)(smax - smin) * 0.5) * invDist with float32 centres; and the sample
   coordinates: the table's float64 node r on the finer side, fl(fl(r invDist) + invT) on the coarser.  The reference itself
   integrates with the Gauss rule proper (the table's nodes refined by Newton in long double: the table holds them rounded, and
   with rounded nodes no rule is exact) and evaluates each leaf at the sample's own unit coordinates x = (q - centre) 2^(d+1),
   q = face centre + node * half extent, in long double; e_x = |product's float64 coordinate - x| is then a known quantity
   and enters the bound through |L_j'| <= j (j + 1) / 2 on [-1, 1].  It is at most K_EX u = 4 u -- the table node's rounding (u |r|
   invDist), the addition's (u |x|), the division and the product that make invT (2 u |invT|), all of magnitude at most 1 -- and the
   reference refuses a pair whose e_x is larger: a wrong sub-face offset or depth factor in the restated lines cannot widen the
   bound.  The table's weights are the rule's rounded: u each.

2. The entrywise bound.  u = 2^-53; first order, times SLACK (hiprec.py) and times LDSLACK = 1 + 2^-10 for the reference's own
   long-double roundings (2^-64 each, i.e. 2^-11 u, at the same places).  A non-conforming (numeric) face contribution is
       v = I_1 I_2 F W,   I_k = sum_q w_q L_a(x_q) L_b(x'_q)  (n terms),   F = L(+-1) L(+-1),   W = scale12 N_i N_j      (|F| = 1)
   (i)   the recurrence model of hiprec.py, |dL_j| <= j^2 u, here of Octree::LpX in float64 with the table's rounded coefficients
         against the Legendre polynomials themselves, at the shifted arguments and at +-1 (tests/test_hiprec_continuity_cpu.py
         checks it there), plus the node term of section 1:   eL_j(q) = j^2 u + j (j + 1) / 2 e_x(q).
         On I_k:  R_k = sum_q |w_q| (eL_a |L_b| + eL_b |L_a|);  on F:  (a_dim^2 + b_dim^2) u.
   (ii)  multiplicative roundings.  Assembler::leafRows: 2 per 1-D term and axis (4), I_1 I_2, fL fO, their product (3), the two
         weights wi, wj (2 + 2), wi wj, scale12, scale12 (wi wj), the last product (4): 15; the final * -1.0 is exact.  The
         reference's tensor loop (:1318-1337, as the oracle restates it): w w and six factors (7), basisWeights (5; 1.0 * N is
         exact), scale scale bw and integral *= (3): 15.  K_NUM = 15 serves both; K_TAB = 2 for the two rounded weights.
   (iii) summation.  leafRows adds n terms per 1-D quadrature in order: (n - 1) u S_k each, S_k = sum_q |w L_a L_b|, hence
         2 (n - 1) u S_1 S_2 on the product.  The tensor loop adds n^2 terms of absolute sum S_1 S_2: (n^2 - 1) u S_1 S_2, which is
         the larger for every n >= 1.  One bound for both evaluation orders:
       |v - v*| <= |W| ( R_1 S_2 + S_1 R_2 + u S_1 S_2 (a_dim^2 + b_dim^2 + n^2 - 1 + K_NUM + K_TAB + 6 K_NL) ).
   (v)   the normalisation.  N_i[d] = sqrt((2 i + 1) 2^d) in the integral; the product reads NormalisedLengths, whose entries are
         within one ulp of it (some are the neighbour of the correctly rounded root): K_NL = 2 u for each of the six factors.
   A conforming (equal-depth) contribution is +-1 L(+-1) N L(+-1) N (:1459-1546): three roundings (K_ANA = 3; +-1.0 * L is exact)
   and the recurrence at +-1:   |v - v*| <= u |v*| (a_dim^2 + b_dim^2 + K_ANA + 2 K_NL);  its in-face integrals are the Kronecker deltas, which
   the reference integrates like any other (the off-diagonal ones come out below 1e-17 and are reported as `offpattern`).
   (iv)  duplicates.  An own-block entry receives one contribution per face of its leaf and adds them in face order starting from
         0.0 (leafRows; setFromTriplets in the reference): k kept contributions pass at most k - 1 roundings of partial sums bounded by
         sum |v|:  + (k - 1) u sum_f |v*_f|.
   An entry's bound is the sum of its kept contributions' bounds plus (iv), plus the undecided ones of section 3.

3. Keep / drop (:1337, :1391, :1448): a numeric contribution is stored iff |(float) v| > 1e-6f.  With T = (double) 1e-6f and
   ulp = 2^-43 (the float32 spacing at T), (float) v > T needs v > T and is certain for v > T + ulp.  Per contribution with bound b:
       keep       |v*| - b > T + ulp                      drop       |v*| + b <= T
   otherwise it is undecided: it stays out of M*, widens the entry's bound by |v*| + b and makes the entry optional in the pattern
   if no kept contribution reaches it.  Conforming entries are stored whenever the transverse indices match.  M* is therefore the
   exact integral minus the dropped contributions D; their magnitudes are kept (`drop`; those below 2^-9 of their own bound, the integrals
   that vanish by orthogonality and are nonzero in long double by rounding alone, are not) because statements about the integral
   (a continuous field has M x = 0, M is positive semidefinite) hold for M* + D:  lambda_min(M* + lambda I) >= lambda - ||D||, with
   ||D|| <= sqrt(||D||_1 ||D||_inf) of the magnitudes (undecided ones included).

4. The solve.  A* = M* + lambda I, b = lambda c, r*(x) = b - A* x in long double.  What the product solved is (M + lambda I) x = fl(b):
       ||r*(x)|| <= tol ||b|| (1 + (n + 2) u) + drift + || B |x| ||_2 + u ||b||,      B the entry bounds,
   ((n + 2) u: the float64 sums r.r and b.b of the stopping rule), where drift bounds the gap g_k = (b - A x_k) - r_k between CG's
   recursive residual and the true one.  One iteration does x += alpha p and r -= alpha tmp with tmp = fl(A p), and
   s_k = alpha_k p_k = x_{k+1} - x_k, so that g_{k+1} - g_k = -A dx + alpha dtmp - dr with, row by row,
       |dx| <= u (|x_{k+1}| + |s_k|),    |alpha dtmp| <= m_i u (|A| |s_k|)_i,    |dr| <= u (|r_{k+1}| + |r_k - r_{k+1}|)
   (m_i = the entries of row i plus the shift's term: m_i products and m_i - 1 additions in any order, which covers both SpMV
   kernels and the host's loop).  The first residual fl(b - fl(A x_0)), x_0 = b (solveWithGuess(rhs, rhs), :1755), starts the gap at
   |g_0| <= u (m_i (|A| |b|)_i + |r_0|).  Hence, with |A| <= |M*| + B + lambda I entrywise,
       drift = u ( || m |A| |b| + |r_0| ||_2 + sum_{k < iterations} || |A| (|x_{k+1}| + |s_k|) + m |A| |s_k| + |r_{k+1}| + |r_k - r_{k+1}| ||_2 ) SLACK.
   It is first order in u, so x_k, s_k and r_k are taken from the long-double Jacobi-PCG of `pcg` (the product's own differ from
   them by terms of order u, which would enter at u^2), for one iteration more than the product reports (the one that meets the
   threshold is not counted).  Nothing in it is a worst case over vectors: |A| acts on the iterates row by row, so a few long or
   badly scaled rows weigh only where the iterates live.
   The tests assert it to be below 1e-2 of tol ||b|| for every case and tolerance they run; its largest part is |g_0|, which is why
   long rows (m) and deep leaves (|A|) raise the tolerance at which that holds.
   The a-posteriori error:  ||x - x*||_2 <= ||r*(x)|| / l,   l = lambda - ||D|| <= lambda_min(A*) (section 3).
   The jump energies of the statistics are x^T M x in float64 (one row sum of at most m terms, one product, a dot of n terms in any
   order):   |jump - x^T M* x| <= |x|^T B |x| + u (m + n + 3) |x|^T |M*| |x|.
"""
import numpy as np

import hiprec as R
from hiprec import LD, COUNT, BIDX, SLACK, U

LDSLACK = 1.0 + 2.0 ** -10
K_NUM, K_ANA, K_TAB = 15, 3, 2
K_EX = 4          # e_x <= 4 u: the node's rounding, the addition's, invT's division and product (every quantity at most 1)
K_NL = 2          # a table entry of NormalisedLengths is within one ulp = 2 u of sqrt((2 i + 1) 2^j)
EPS_F32 = np.float32(0.000001)           # Include/Utility/Literals.h:14
T_KEEP = float(EPS_F32)
T_ULP = float(np.spacing(EPS_F32))
KEEP, DROP, UNDECIDED = 0, 1, 2
MUTANTS = ("face_swap", "invT_neg", "invDist_dm1", "scale12_coarse", "nl_other_depth", "skip_fine_neighbour", "gauss_short")


def legendre(x, p):
    """The Legendre polynomials P_0..P_p at long-double arguments, by Bonnet's recurrence with its exact coefficients (the table's
    (2j - 1) / j and (j - 1) / j are these rounded to float64: one more rounding of the product's, inside the j^2 u model)
    -> [p + 1, len(x)] long double."""
    x = np.asarray(x, LD)
    out = np.empty((p + 1,) + x.shape, LD)
    m2, m1 = np.zeros_like(x), np.ones_like(x)
    out[0] = 1
    for j in range(1, p + 1):
        li = ((2 * j - 1) * x * m1 - (j - 1) * m2) / j
        m2, m1 = m1, li
        out[j] = li
    return out


# N_i[d] = sqrt((2 i + 1) 2^d): the normalisation itself (the table holds it to one ulp, tests/test_hiprec_cpu.py)
NL_LD = np.sqrt(((2 * np.arange(13, dtype=np.int64)[:, None] + 1) * 2 ** np.arange(11, dtype=np.int64)[None, :]).astype(LD))
_RULES = {}


def rule_ld(n):
    """The Gauss-Legendre rule of order n to long-double accuracy: Newton on P_n from the table's float64 nodes, weights
    2 / ((1 - x^2) P_n'(x)^2) -> (nodes, weights) long double.  (tests/test_hiprec_cpu.py shows the table to be these, rounded.)"""
    if n not in _RULES:
        x = R.rule(n)[0].astype(LD)
        for _ in range(4):
            p0, p1 = np.ones_like(x), x.copy()
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            d = n * (x * p1 - p0) / (x * x - 1)
            x = x - p1 / d
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        d = n * (x * p1 - p0) / (x * x - 1)
        _RULES[n] = (x, 2 / ((1 - x * x) * d * d))
    return _RULES[n]


def with_strength(blk, strength):
    """The block with continuity.strength set in its config (the last 80 bytes; the double at offset 24)."""
    b = bytearray(blk)
    b[-80 + 24:-80 + 32] = np.array([strength], np.float64).tobytes()
    return bytes(b)


def strength_of(blk):
    return float(np.frombuffer(bytes(blk)[-80 + 24:-80 + 32], np.float64)[0])


# ---------------------------------------------------------------------------------------------------------------- pairs
def face_pairs(blk):
    """Every (A, B, dim) of leaves whose float32 boxes touch across a plane normal to dim (A below it) and overlap with positive
    area in the other two dimensions.  Leaves are grouped by the plane's coordinate (a sort), overlaps tested within a group."""
    lv = blk.leaves()
    out = []
    for dim in range(3):
        hi, lo = blk.bmax[lv, dim], blk.bmin[lv, dim]
        oh, ol = np.argsort(hi, kind="stable"), np.argsort(lo, kind="stable")
        for pl in np.intersect1d(hi, lo):
            A = lv[oh[np.searchsorted(hi[oh], pl, "left"):np.searchsorted(hi[oh], pl, "right")]]
            B = lv[ol[np.searchsorted(lo[ol], pl, "left"):np.searchsorted(lo[ol], pl, "right")]]
            ov = np.ones((len(A), len(B)), bool)
            for m in ((dim + 1) % 3, (dim + 2) % 3):
                l = np.maximum(blk.bmin[A, m][:, None], blk.bmin[B, m][None, :])
                h = np.minimum(blk.bmax[A, m][:, None], blk.bmax[B, m][None, :])
                ov &= h > l
            ia, ib = np.nonzero(ov)
            out += [(int(A[i]), int(B[j]), dim) for i, j in zip(ia, ib)]
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- one pair
def _pair(blk, A, B, dim, mut, cache):
    """The contributions of one pair -> list of (rows, cols, val [LD], bound, status) and the largest off-pattern conforming value.
    Everything after the bit-for-bit quantities of section 1 depends on the pair only through them, the degrees, the depths and
    the face's position in each leaf's unit coordinates: pairs that agree in all of these share one evaluation (`cache`)."""
    m1, m2 = (dim + 1) % 3, (dim + 2) % 3
    dA, dB = int(blk.depth[A]), int(blk.depth[B])
    pA, pB = int(blk.degree[A]), int(blk.degree[B])
    numeric = dA != dB
    # section 1, bit for bit: :1264-1266
    lo = np.maximum(blk.bmin[A], blk.bmin[B])
    hi = np.minimum(blk.bmax[A], blk.bmax[B])
    scale = (hi - lo).astype(np.float64) * 0.5
    if mut == "scale12_coarse" and numeric:
        c = A if dA < dB else B
        scale = (blk.bmax[c] - blk.bmin[c]).astype(np.float64) * 0.5
    dd = abs(dA - dB)
    inv_dist = 1.0 / 2.0 ** (dd - 1 if (mut == "invDist_dm1" and numeric) else dd)        # :1275
    s, l = (A, B) if dA > dB else (B, A)                                                   # the deeper cell, the other
    inv_t = [0.0, 0.0]
    for k, m in enumerate((m1, m2)):                                                       # :1278-1290
        cs = (blk.bmin[s, m] + blk.bmax[s, m]) / np.float32(2.0)
        cl = (blk.bmin[l, m] + blk.bmax[l, m]) / np.float32(2.0)
        inv_t[k] = float(np.float64(cs - cl) / (np.float64(blk.bmax[s, m] - blk.bmin[s, m]) * 0.5) * inv_dist)
    if mut == "invT_neg":
        inv_t[0] = -inv_t[0]
    # as Query, :862: x = (q - centre) 2^(d+1) at q = face centre + node * half extent = off + node * sc, distributed so that the
    # only rounding is that last addition (the differences and the products by powers of two are exact in long double)
    geo = []
    for node, dep in ((A, dA), (B, dB)):
        cen = ((blk.bmin[node] + blk.bmax[node]) / np.float32(2.0)).astype(np.float64)
        for m in (m1, m2):
            geo.append((float(((LD(lo[m]) + LD(hi[m])) / 2 - LD(cen[m])) * LD(float(2 << dep))), float(LD(scale[m]) * LD(float(2 << dep)))))
    key = (pA, pB, dA, dB, dim, float(scale[m1]), float(scale[m2]), inv_dist, inv_t[0], inv_t[1], tuple(geo))
    if key not in cache:
        cache[key] = _blocks(*key, mut)
    blocks, off = cache[key]
    start = {"A": int(blk.start[A]), "B": int(blk.start[B])}
    out = []
    count = 0
    for X, Y, ii, jj, v, b, st, cnt in blocks:
        rows, cols = start[X] + ii, start[Y] + jj
        out.append((rows, cols, v, b, st))
        count += cnt
        if X != Y:
            out.append((cols, rows, v, b, st))
            count += cnt
    return out, off, count


def _blocks(pA, pB, dA, dB, dim, scale1, scale2, inv_dist, inv_t1, inv_t2, geo, mut):
    m1, m2 = (dim + 1) % 3, (dim + 2) % 3
    numeric = dA != dB
    pmax = max(pA, pB)
    n = pmax + 1
    if mut == "gauss_short":
        n = max(1, pmax)
    r, w = R.rule(n)                     # the table's float64 rule: what the product samples at
    rl, wl = rule_ld(n)                  # the rule itself: what the reference integrates with
    scale12 = scale1 * scale2
    inv_t = {m1: inv_t1, m2: inv_t2}
    formula = mut in ("invT_neg", "invDist_dm1")
    # per side and in-face axis: L at the samples, and eL (section 2 (i))
    L, eL = {}, {}
    for si, (side, dep, deg) in enumerate((("A", dA, pA), ("B", dB, pB))):
        coarse = numeric and dep < max(dA, dB)
        for k, m in enumerate((m1, m2)):
            off_, sc = geo[2 * si + k]
            x = LD(off_) + rl * LD(sc)
            xp = (r * inv_dist + inv_t[m]) if coarse else r                                # the product's float64 coordinate
            if formula:
                x = rl * LD(inv_dist) + LD(inv_t[m]) if coarse else rl
            ex = np.abs(xp.astype(LD) - x).astype(np.float64) if not formula else np.zeros(n)
            # section 1: the restated invDist / invT must land on the geometric coordinate, or the bound would absorb their error
            assert mut is not None or (ex <= K_EX * U * LDSLACK).all(), (ex.max() / U, dA, dB, inv_dist, inv_t[m])
            j = np.arange(deg + 1, dtype=np.float64)[:, None]
            L[side, m] = legendre(x, deg)
            eL[side, m] = j * j * U + j * (j + 1) / 2 * ex[None, :]
    one = legendre(np.array([1, -1], LD), 12)                                               # L_j(+1), L_j(-1)
    face = {"A": one[:, 0], "B": one[:, 1]}
    if mut == "face_swap":
        face = {"A": one[:, 1], "B": one[:, 0]}
    dep_of = {"A": dA, "B": dB}
    if mut == "nl_other_depth":
        dep_of = {"A": dB, "B": dA}
    idx = {"A": BIDX[:int(COUNT[pA])], "B": BIDX[:int(COUNT[pB])]}
    Nw = {sd: (NL_LD[idx[sd][:, 0], dep_of[sd]] * NL_LD[idx[sd][:, 1], dep_of[sd]] * NL_LD[idx[sd][:, 2], dep_of[sd]]) for sd in "AB"}
    out, off = [], 0.0
    for X, Y, sign in (("A", "A", 1), ("B", "B", 1), ("A", "B", -1)):
        bx, by = idx[X], idx[Y]
        I, S, Rr = {}, {}, {}
        for m in (m1, m2):
            lx, ly = L[X, m], L[Y, m]
            I[m] = (lx * wl[None, :]) @ ly.T
            ax, ay = np.abs(lx).astype(np.float64), np.abs(ly).astype(np.float64)
            aw = np.abs(w)
            S[m] = (ax * aw[None, :]) @ ay.T
            Rr[m] = (eL[X, m] * aw[None, :]) @ ay.T + (ax * aw[None, :]) @ eL[Y, m].T
        g1 = (bx[:, m1][:, None], by[:, m1][None, :])
        g2 = (bx[:, m2][:, None], by[:, m2][None, :])
        F = face[X][bx[:, dim]][:, None] * face[Y][by[:, dim]][None, :]
        W = LD(scale12) * Nw[X][:, None] * Nw[Y][None, :]
        val = LD(sign) * I[m1][g1] * I[m2][g2] * F * W
        d2 = (bx[:, dim].astype(np.float64) ** 2)[:, None] + (by[:, dim].astype(np.float64) ** 2)[None, :]
        if numeric:
            Wa = np.abs(W).astype(np.float64)
            bound = Wa * (Rr[m1][g1] * S[m2][g2] + S[m1][g1] * Rr[m2][g2] + U * S[m1][g1] * S[m2][g2] * (d2 + n * n - 1 + K_NUM + K_TAB + 6 * K_NL))
            av = np.abs(val).astype(np.float64)
            status = np.full(val.shape, UNDECIDED, np.int8)
            status[av - bound > T_KEEP + T_ULP] = KEEP
            status[av + bound <= T_KEEP] = DROP
            sel = np.ones(val.shape, bool)
        else:
            sel = (g1[0] == g1[1]) & (g2[0] == g2[1])
            if (~sel).any():
                off = max(off, float(np.abs(val[~sel]).max()))
            bound = U * np.abs(val).astype(np.float64) * (d2 + K_ANA + 2 * K_NL)
            status = np.full(val.shape, KEEP, np.int8)
        # (an integral that vanishes by orthogonality comes out at long-double rounding level, which LDSLACK puts below 2^-10 of
        # the bound: a dropped contribution below 2^-9 of its own bound is not recorded)
        ii, jj = np.nonzero(sel & ((status != DROP) | (np.abs(val).astype(np.float64) > 2.0 ** -9 * bound)))
        out.append((X, Y, ii, jj, val[ii, jj], bound[ii, jj], status[ii, jj], int(sel.sum())))
    return out, off


# ---------------------------------------------------------------------------------------------------------------- the matrix
class Reference:
    """M* in coordinate form, sorted by (row, column): val (kept contributions, long double), bound, must / opt (the pattern),
    drop (magnitude of what the keep/drop rule left out or could not decide)."""

    def matvec(self, x, weights=None):
        """sum_j w_ij x_j per row; weights default to val (long double), else a float64 array over the entries."""
        wv = self.val if weights is None else weights
        prod = wv * np.asarray(x)[self.col]
        y = np.zeros(self.n, prod.dtype)
        ne = self.rp[1:] > self.rp[:-1]
        if ne.any():
            y[ne] = np.add.reduceat(prod, self.rp[:-1][ne])
        return y

    def compare(self, rp, ci, v):
        """A CSR matrix against M* -> (largest |v - v*| / bound, entries outside must | opt, must entries missing)."""
        rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(rp))
        key = rows * self.n + ci
        at = np.minimum(np.searchsorted(self.key, key), max(len(self.key) - 1, 0))
        found = (self.key[at] == key) if len(self.key) else np.zeros(len(key), bool)
        allowed = found & (self.must | self.opt)[at] if len(self.key) else found
        missing = int((~np.isin(self.key[self.must], key)).sum())
        ratio = 0.0
        if allowed.any():
            d = np.abs(np.asarray(v, np.float64)[allowed].astype(LD) - self.val[at[allowed]]).astype(np.float64)
            ratio = float((d / self.bound[at[allowed]]).max())
        return ratio, int((~allowed).sum()), missing

    def jump(self, x):
        """x^T M* x and the bound of section 4 for the statistics' float64 value."""
        xl = np.asarray(x, np.float64).astype(LD)
        xa = np.abs(np.asarray(x, np.float64))
        val = (xl * self.matvec(xl)).sum()
        b = (xa * self.matvec(xa, self.bound)).sum() + U * (self.m + self.n + 3) * (xa * self.matvec(xa, self.aval)).sum()
        return val, float(b) * SLACK * LDSLACK

    def residual(self, x, c, lam):
        """r*(x) = lam c - (M* + lam I) x in long double (x float64 or long double)."""
        return LD(lam) * np.asarray(c, np.float64).astype(LD) - self.apply(np.asarray(x).astype(LD), lam)

    def apply(self, x, lam):
        return self.matvec(x) + LD(lam) * x

    def energy(self, e, lam):
        return (e * self.apply(e, lam)).sum()


def _coalesce(key, arrays):
    """Sums each array over equal keys -> (unique keys, summed arrays, counts)."""
    order = np.argsort(key, kind="stable")
    key = key[order]
    first = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if len(key) else np.zeros(0, np.int64)
    sums = [np.add.reduceat(a[order], first) if len(key) else a[:0] for a in arrays]
    cnt = np.diff(np.concatenate([first, [len(key)]]))
    return key[first] if len(key) else key, sums, cnt


def reference(block, mut=None):
    blk = block if isinstance(block, R.Block) else R.Block(block)
    n = len(blk.coeffs)
    pairs = face_pairs(blk)
    numeric = [blk.depth[a] != blk.depth[b] for a, b, _ in pairs]
    if mut == "skip_fine_neighbour" and any(numeric):
        pairs = list(pairs)
        del pairs[numeric.index(True)]
    parts, off, cache, ncontrib = [], 0.0, {}, 0
    for a, b, dim in pairs:
        got, o, cnt = _pair(blk, a, b, dim, mut, cache)
        parts += got
        off = max(off, o)
        ncontrib += cnt
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    rows, cols, val, bnd, st = cat(0, np.int64), cat(1, np.int64), cat(2, LD), cat(3, np.float64), cat(4, np.int8)
    key = rows * n + cols
    av = np.abs(val).astype(np.float64)
    k = st == KEEP
    kk, (kv, kb, ka), kc = _coalesce(key[k], [val[k], bnd[k], av[k]])
    kb = kb + U * (kc - 1) * ka                                         # section 2 (iv)
    u_ = st == UNDECIDED
    uk, (uw,), _ = _coalesce(key[u_], [av[u_] + bnd[u_]])
    d_ = st == DROP
    dk, (dw,), _ = _coalesce(key[d_], [av[d_]])
    allk = np.union1d(np.union1d(kk, uk), dk)
    ref = Reference()
    ref.n, ref.key = n, allk
    ref.row, ref.col = allk // max(n, 1), allk % max(n, 1)
    ref.val, ref.bound, ref.drop = np.zeros(len(allk), LD), np.zeros(len(allk)), np.zeros(len(allk))
    ref.must, ref.opt = np.zeros(len(allk), bool), np.zeros(len(allk), bool)
    ik, iu, id_ = np.searchsorted(allk, kk), np.searchsorted(allk, uk), np.searchsorted(allk, dk)
    ref.val[ik], ref.must[ik] = kv, True
    ref.bound[ik] = kb
    ref.bound[iu] += uw
    ref.opt[iu] = True
    ref.opt &= ~ref.must
    ref.drop[id_] += dw
    ref.drop[iu] += uw
    ref.bound *= SLACK * LDSLACK
    ref.aval = np.abs(ref.val).astype(np.float64)
    ref.rp = np.searchsorted(ref.row, np.arange(n + 1))
    ref.n_pairs, ref.n_numeric = len(pairs), int(sum(blk.depth[a] != blk.depth[b] for a, b, _ in pairs))
    ref.n_analytic = ref.n_pairs - ref.n_numeric
    ref.n_contrib, ref.n_undecided = ncontrib, int(u_.sum())
    ref.offpattern = off
    ref.nnz = int(ref.must.sum())
    stored = np.bincount(ref.row[ref.must], minlength=n) if n else np.zeros(0, np.int64)
    ref.longest_row = int(stored.max()) if n and len(stored) else 0
    ref.m = ref.longest_row + int(np.bincount(ref.row[ref.opt], minlength=n).max() if ref.opt.any() else 0) + 1
    ones = np.ones(n)
    dr = ref.matvec(ones, ref.drop)
    dc = np.bincount(ref.col, ref.drop, minlength=n) if len(allk) else np.zeros(n)
    ref.drop_norm = float(np.sqrt(dr.max() * dc.max())) if n and len(allk) else 0.0
    return ref


# ---------------------------------------------------------------------------------------------------------------- the solve
def pcg(ref, c, lam, iters, keep=()):
    """Textbook Jacobi-preconditioned CG on A* x = lam c from x_0 = lam c, in long double -> (x, {k: x_k for k in keep})."""
    b = LD(lam) * np.asarray(c, np.float64).astype(LD)
    diag = np.full(ref.n, LD(lam))
    on = ref.row == ref.col
    diag[ref.row[on]] += ref.val[on]
    x = b.copy()
    r = b - ref.apply(x, lam)
    z = r / diag
    p = z.copy()
    rz = (r * z).sum()
    got = {0: x.copy()} if 0 in keep else {}
    for k in range(1, iters + 1):
        if rz == 0:
            break
        ap = ref.apply(p, lam)
        alpha = rz / (p * ap).sum()
        x = x + alpha * p
        r = r - alpha * ap
        if k in keep:
            got[k] = x.copy()
        z = r / diag
        rz_new = (r * z).sum()
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, got


def cg_drift(ref, c, lam, iters):
    """The drift term of section 4 after `iters` iterations, evaluated along the long-double PCG iterates (cached per reference,
    right-hand side and strength: the cumulative sums of one run serve every shorter one)."""
    c = np.asarray(c, np.float64)
    tag = (c.tobytes(), float(lam))
    cache = ref.__dict__.setdefault("_drift", {})
    if tag not in cache or len(cache[tag]) <= iters:
        b = LD(lam) * c.astype(LD)
        diag = np.full(ref.n, LD(lam))
        on = ref.row == ref.col
        diag[ref.row[on]] += ref.val[on]
        wabs = ref.aval + ref.bound
        absA = lambda v: ref.matvec(v, wabs) + lam * v                                      # |A| v for v >= 0, float64
        m = np.bincount(ref.row[ref.must | ref.opt], minlength=ref.n).astype(np.float64) + 1
        f64 = lambda v: np.abs(v).astype(np.float64)
        x = b.copy()
        r = b - ref.apply(x, lam)
        z = r / diag
        p = z.copy()
        rz = (r * z).sum()
        cum = [norm2(m * absA(f64(b)) + f64(r))]
        for _ in range(iters):
            if rz == 0:
                cum.append(cum[-1])
                continue
            ap = ref.apply(p, lam)
            alpha = rz / (p * ap).sum()
            s, dr = alpha * p, alpha * ap
            x, r = x + s, r - dr
            sa = f64(s)
            cum.append(cum[-1] + norm2(absA(f64(x) + sa) + m * absA(sa) + f64(r) + f64(dr)))
            z = r / diag
            rz_new = (r * z).sum()
            p = z + (rz_new / rz) * p
            rz = rz_new
        cache[tag] = cum
    return U * cache[tag][iters] * SLACK


def solve(ref, c, lam, dense_limit=5000):
    """x* of A* x = lam c: an LU solve in float64 and long-double refinement (n <= dense_limit), else long-double CG; with the
    bound ||r*(x*)|| / (lam - ||D||) on its own error."""
    cl = np.asarray(c, np.float64)
    if ref.n <= dense_limit:
        import scipy.linalg as sl
        A = np.zeros((ref.n, ref.n))
        A[ref.row, ref.col] = ref.val.astype(np.float64)
        A[np.arange(ref.n), np.arange(ref.n)] += lam
        lu = sl.lu_factor(A)
        x = sl.lu_solve(lu, lam * cl).astype(LD)
        for _ in range(2):
            x = x + sl.lu_solve(lu, ref.residual(x, cl, lam).astype(np.float64)).astype(LD)
    else:
        x, _ = pcg(ref, cl, lam, 4 * ref.n)
    own = float(np.sqrt((ref.residual(x, cl, lam) ** 2).sum())) / (lam - ref.drop_norm)
    return x, own


def norm2(v):
    return float(np.sqrt((np.asarray(v, LD) ** 2).sum()))


def solve_figures(ref, blk_in, blk_out, stats, tol):
    """The figures of section 4 for one post-process: blk_in -> blk_out with `stats`, stopped at `tol` (0: the default 1e-6f)."""
    c, x = R.Block(blk_in).coeffs, R.Block(blk_out).coeffs
    lam = strength_of(blk_in)
    l = lam - ref.drop_norm
    tol = T_KEEP if not tol > 0 else tol
    b = norm2(lam * c.astype(LD))
    matrix = norm2(ref.matvec(np.abs(x), ref.bound))
    rn = norm2(ref.residual(x, c, lam))
    drift = cg_drift(ref, c, lam, int(stats["iterations"]) + 1)      # the update that met the threshold is not counted
    stop = tol * b * (1 + (ref.n + 2) * U)
    jb, jbb = ref.jump(c)
    ja, jab = ref.jump(x)
    return {"lam": lam, "l": l, "b": b, "res": rn, "allowed": stop + drift + matrix + U * b, "stop": stop, "drift": drift,
            "matrix": matrix, "err_bound": rn / l,
            "jump_before": abs(float(LD(stats["jump_before"]) - jb)) / jbb if jbb > 0 else float(jb != stats["jump_before"]),
            "jump_after": abs(float(LD(stats["jump_after"]) - ja)) / jab if jab > 0 else float(ja != stats["jump_after"]),
            "x": x, "c": c}
