"""Nearness weighting (Config::nearnessWeighting, Octree.cpp:1071-1092 and :1209-1247) in extended precision, for the build replay of
tests/hiprec_build.py: the weight of every fit that steers a weighted build, with a bound, independent of the oracle and of the
product.  It is written from Octree.cpp (CalculatePolyWeighting :1209-1227, CalculateExpWeighting :1230-1247, FApprox :859-901,
the copy of the old rows in EstimatePImprovement :847) and from the definition of the sample generator below.

Notation as in hiprec.py: u = 2^-53, fl(a op b) = (a op b)(1 + d) with |d| <= u, first-order bounds times SLACK = 1 + 1e-6.
No number below was chosen by looking at a kernel's or the oracle's output.

1. The sample points.  The reference draws 100 points with AlignedBox3f::sample(), that is std::rand: different from run to run.
   This project replaces the generator, and nothing else, by a pure function of (cell, depth, degree, sample, axis)
   (DESIGN.md section 2).  Its definition, restated here and not imported:
       sm(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
               return z ^ (z >> 31)                                  (SplitMix64; all arithmetic modulo 2^64)
       key   = sm(bits(bmin.x) | bits(bmin.y) << 32)  ^  sm((bits(bmin.z) | depth << 32 | degree << 40) ^ 0xD1B54A32D192ED03)
       r     = f32(sm(key + (3 n + a) * 0x9E3779B97F4A7C15) >> 40) * 2^-24        sample n = 0..99, axis a = 0..2
       pt    = f32(bmin + f32(f32(bmax - bmin) * r))                 (float32, no contraction: AlignedBox3f::sample())
   bits() is the float32's bit pattern, `degree` the degree of the fit being weighted: p + 1 for the P fit of a node of degree
   p, p for a child, 2 for a coarse job; `depth` is that fit's depth.  The 24-bit integer is exact in float32 and so is its
   product with 2^-24: r is k 2^-24 with 0 <= k < 2^24, hence 0 <= r < 1 and bmin <= pt <= bmax (rounding is monotone).
   Then the reference's mapping (:862, with the float32 centre of :1021):
       x = (f64(pt) - f64(f32(f32(bmin + bmax) / 2))) * (2 << depth)
   in float64.  A cell of the build is dyadic: bmin is a multiple of its extent 2^-depth, so f32(ext * r) and pt are multiples of
   2^-(24 + depth) below 1 in magnitude, the centre is a multiple of 2^-(depth + 1): the difference has at most 35 significant
   bits and is exact in float64, and the scale is a power of two.  So x is an exact statement, the device's x bit for bit, and
   |x| <= 1.  sample_points() computes it in numpy uint64 / float32 / float64 and asserts the exactness against long double.

2. The mean.  m = |(1 / 100) sum_n f(x_n)| (:1216-1222), f the polynomial of :859-901 with the array's coefficients.  The
   reference value is the long-double mean of the long-double polynomial whose coefficients are the ones the fit history gives
   that array (hiprec_build.py section 5): a from-scratch array of degree p0 is fit_reference's of degree p0; a P array of degree
   q is the node's rows -- rows below COUNT[p0] from the degree-p0 fit, rows COUNT[j - 1] .. COUNT[j] - 1 from the degree-j fit,
   j = p0 + 1 .. q - 1, copied (:847) -- plus rows COUNT[q - 1] .. COUNT[q] - 1 from the degree-q fit.  Its bound, per term:
   (a) the coefficients.  The float64 array differs from the reference row by row by at most the row's fit bound b_i
       (hiprec.py section 2), so f(x_n) moves by at most sum_i b_i N_i |L_a(x) L_b(y) L_c(z)|, N_i = N_a N_b N_c at the fit's depth.
   (b) the float64 evaluation at x_n: hiprec.py section 3 as it stands (the recurrence's j^2 u, K_Q = 6 roundings a term, the
       partial sums in the loop's order), u (sum_i |c_i| N_i (a^2 |L_b L_c| + b^2 |L_a L_c| + c^2 |L_a L_b| + K_Q |L_a L_b L_c|)
       + sum_{i >= 1} |s_i|).
   (c) the 100 additions in the loop's order (:1217-1220; the first, to 0.0, is exact) and the division by 100.0:
       u sum_{k = 1..99} |S_k| with S_k the exact partial sums over the samples, then u |mean| for the quotient.
       d(mean) = ((1 / 100) sum_n ((a)_n + (b)_n) + (u / 100) sum_k |S_k| + u |mean|) SLACK.
   abs is 1-Lipschitz: d(m) = d(mean).

3. The weight.  d = sqrt(3.0) in float64 is sqrt 3 correctly rounded (relative u); the reference value uses the long-double root.
   Polynomial (:1225-1226):  q = m / d, base = fl(1 - q), k = pow(base, s), w = min(1, max(k, 0)).
       d(q) = d(m) / d + 2u q                 (the rounded d and the division)
       d(base) = d(q) + u |base|
       d(k) = s (|base| + d(base))^(s - 1) d(base) + P u' |k|      for s >= 1 (the derivative is monotone in |base|)
   with P = 1 the error of glibc's pow in ulp and u' = 2u the relative size of an ulp at most.  P = 1 (and E = 1 for exp) are the
   figures of the glibc manual's table "Known Maximum Errors in Math Functions" for x86_64 double; the host forms every weight
   with glibc (csrc/builder.hpp nearnessWeight, for both schedulers), the oracle likewise.  max and min are 1-Lipschitz: d(w) = d(k).
   The reference's own edge semantics, reproduced:
       m > sqrt 3 makes base < 0.  An odd integer strength (3, the reference's) gives k < 0 and w = 0 exactly; an even integer
       gives k = |base|^s clamped at 1.  A fractional strength gives pow = NaN; std::max<f64>(NaN, 0.0) returns its first
       argument, NaN, and std::min<f64>(1.0, NaN) its first, 1.0: the weight is 1.
       With a fractional strength, |base| <= d(base) cannot tell the NaN branch from the real one, and for s < 1 the derivative
       is unbounded there.  Such a fit is UNDECIDED by construction: its bound is infinite and it is counted ("excluded").  For
       s < 1 away from it the derivative is taken at |base| - d(base).
   Exponential (:1246):  w = exp(fl(fl(-1.0 s) m) / d); -1.0 s is exact, the product, the division and d round once each:
       d(arg) = s d(m) / d + 3u |arg|,    d(w) = w d(arg) + E u' w.
   The weighted error (:1080, :1085) is fl(e w):  d(e w) = w d(e) + e d(w) + d(e) d(w) + u |e w|.

4. Which fits are weighted (hiprec_build.py section 2).  Each of a job's nine errors with its own array: p_err with the P array
   (key degree p + 1, the job's cell and depth), h_err[i] with child i's from-scratch array (key degree p, the child's cell, depth
   d + 1).  A coarse job weights p_err alone with its degree-2 array; its eight other header slots belong to no fit and stay 0.
"""
import numpy as np

import hiprec as R

LD, U, SLACK = R.LD, R.U, R.SLACK
COUNT, BIDX, NL = R.COUNT, R.BIDX, R.NL
NONE, POLYNOMIAL, EXPONENTIAL = 0, 1, 2
N_SAMPLES = 100
POW_ULP = EXP_ULP = 1.0
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUTANTS = ("w_new_rows", "w_child_parent", "w_coarse_nine", "w_d3", "w_noabs", "w_noclamp", "w_exp_plus", "w_99", "w_shift1",
           "w_key_nodegree")


# ---------------------------------------------------------------------------------------------------------------- the sampler
def splitmix64(z):
    z = np.asarray(z, np.uint64) + GOLDEN
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def weight_key(bmin, depth, degree):
    """Section 1's key for cells bmin ([C, 3] float32) -> [C] uint64."""
    b = np.ascontiguousarray(np.atleast_2d(np.asarray(bmin, np.float32))).view(np.uint32).astype(np.uint64)
    ka = b[:, 0] | (b[:, 1] << np.uint64(32))
    kb = b[:, 2] | (np.uint64(int(depth)) << np.uint64(32)) | (np.uint64(int(degree)) << np.uint64(40))
    return splitmix64(ka) ^ splitmix64(kb ^ np.uint64(0xD1B54A32D192ED03))


def sample_points(bmin, bmax, depth, degree, count=N_SAMPLES, shift=2, key_degree=True):
    """Section 1 for cells bmin, bmax ([C, 3] float32) -> (pt [C, count, 3] float32, x [C, count, 3] float64)."""
    lo = np.atleast_2d(np.asarray(bmin, np.float32))
    hi = np.atleast_2d(np.asarray(bmax, np.float32))
    key = weight_key(lo, depth, degree if key_degree else 0)
    n = np.arange(count, dtype=np.uint64)[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None, :]
    z = splitmix64(key[:, None, None] + n[None] * GOLDEN)
    r = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    ext = (hi - lo).astype(np.float32)
    pt = (lo[:, None, :] + (ext[:, None, :] * r).astype(np.float32)).astype(np.float32)
    centre = ((lo + hi) / np.float32(2.0)).astype(np.float32)
    x = (pt.astype(np.float64) - centre.astype(np.float64)[:, None, :]) * float(shift << int(depth))
    exact = (pt.astype(LD) - centre.astype(LD)[:, None, :]) * LD(shift << int(depth))
    assert np.array_equal(x.astype(LD), exact), "the mapping of :862 is not exact in float64 for this cell"
    return pt, x


# ---------------------------------------------------------------------------------------------------------------- the mean
def mean_reference(coeffs, cbound, x, degree, depth):
    """Section 2 for A arrays of one degree and depth: coeffs [A, COUNT[degree]] long double, cbound [A, COUNT[degree]] float64
    (the rows' fit bounds, 0 for float64 coefficients taken as given), x [A, n, 3] float64 -> (signed mean [A] long double,
    bound [A])."""
    nc = int(COUNT[degree])
    a, b, c = BIDX[:nc, 0], BIDX[:nc, 1], BIDX[:nc, 2]
    Nd = NL[:degree + 1, depth].astype(LD)
    L = [R.legendre_ld(x[:, :, k], degree) for k in range(3)]                   # [degree + 1, A, n]
    Lf = [L[k] * Nd[:, None, None] for k in range(3)]
    La = [np.abs(L[k]).astype(np.float64) for k in range(3)]
    co = np.asarray(coeffs, LD)
    t = co.T[:, :, None] * Lf[0][a] * Lf[1][b] * Lf[2][c]                       # [nc, A, n]
    s = np.cumsum(t, axis=0)
    f = s[-1]                                                                   # [A, n]
    Nf = (Nd[a] * Nd[b] * Nd[c]).astype(np.float64)[:, None, None]
    lll = La[0][a] * La[1][b] * La[2][c]
    rec = (a ** 2)[:, None, None] * La[1][b] * La[2][c] + (b ** 2)[:, None, None] * La[0][a] * La[2][c] \
        + (c ** 2)[:, None, None] * La[0][a] * La[1][b]
    ca = np.abs(co).astype(np.float64).T[:, :, None]
    cb = np.asarray(cbound, np.float64).T[:, :, None]
    term_a = (cb * Nf * lll).sum(0)                                             # [A, n]
    term_b = U * ((ca * Nf * (rec + R.K_Q * lll)).sum(0) + np.abs(s[1:]).astype(np.float64).sum(0))
    S = np.cumsum(f, axis=1)
    n = x.shape[1]
    mean = S[:, -1] / LD(n)
    bound = ((term_a + term_b).sum(1) / n + U * np.abs(S[:, 1:]).astype(np.float64).sum(1) / n + U * np.abs(mean).astype(np.float64)) * SLACK
    return mean, bound


# ---------------------------------------------------------------------------------------------------------------- the weight
def weight_from_mean(wtype, strength, mean, mean_bound, mutant=None):
    """Section 3 from the signed long-double mean and its bound -> (w long double, bound, tag); tag is "zero" (base < 0, weight 0
    exactly), "nan" (the NaN branch: weight 1), "excluded" (undecided by construction: the bound is infinite) or ""."""
    s = float(strength)
    m = LD(mean) if mutant == "w_noabs" else abs(LD(mean))
    d = LD(3) if mutant == "w_d3" else np.sqrt(LD(3))
    q = m / d
    dq = mean_bound / float(d) + 2 * U * float(abs(q))
    if wtype == EXPONENTIAL:
        arg = (LD(s) if mutant == "w_exp_plus" else -LD(s)) * q
        darg = s * mean_bound / float(d) + 3 * U * float(abs(arg))
        w = np.exp(arg)
        return w, (float(w) * darg + EXP_ULP * 2 * U * float(w)) * SLACK, ""
    assert wtype == POLYNOMIAL
    base = LD(1) - q
    db = dq + U * float(abs(base))
    ab = float(abs(base))
    integer = s.is_integer()
    if not integer and ab <= db:
        return LD(1), np.inf, "excluded"
    if base < 0 and not integer:
        return (LD(np.nan) if mutant == "w_noclamp" else LD(1)), 0.0, "nan"
    k = abs(base) ** LD(s)
    if base < 0 and int(s) % 2 == 1:
        k = -k
    slope = s * (ab + db) ** (s - 1) if s >= 1 else s * (ab - db) ** (s - 1)
    dk = (slope * db + POW_ULP * 2 * U * float(abs(k))) * SLACK
    w = k if mutant == "w_noclamp" else min(LD(1), max(k, LD(0)))
    return w, dk, "zero" if (base < 0 and w == 0) else ""


def weighted_error(e, e_bound, w, w_bound):
    """fl(e w) with section 3's bound -> (value long double, bound)."""
    v = LD(e) * LD(w)
    if not np.isfinite(w_bound):
        return v, np.inf
    return v, (float(abs(w)) * e_bound + float(abs(e)) * w_bound + e_bound * w_bound + U * float(abs(v))) * SLACK


# ---------------------------------------------------------------------------------------------------------------- arrays of a build
class Weighting:
    """The weights of a build's fit arrays, computed in batches and cached.  An array is named by (bmin, bmax, depth, p0, p, kind):
    the cell, the fit's depth, the degree p0 of the from-scratch fit that began the array, its degree p now, and kind "P" (the P
    array of a job: old rows and appended rows), "H" (a child's from-scratch array, p0 == p) or "C" (a coarse job's, p0 == p == 2)."""

    def __init__(self, wtype, strength, mutant=None):
        assert wtype in (POLYNOMIAL, EXPONENTIAL) and strength > 0          # Config.cpp:23-25
        self.wtype, self.strength, self.mutant = int(wtype), float(strength), mutant
        self.cache = {}
        self.seen = {"arrays": 0, "zero": 0, "nan": 0, "excluded": 0, "max_degree": 0, "appends_carried": 0}

    @staticmethod
    def key(lo, hi, depth, p0, p, kind):
        return (np.asarray(lo, np.float32).tobytes() + np.asarray(hi, np.float32).tobytes(), int(depth), int(p0), int(p), kind)

    def array(self, fits, lo, hi, depth, p0, p, kind):
        """Section 2's coefficients and their bounds for one array -> ([COUNT[p]] long double, [COUNT[p]] float64)."""
        co, cb = np.zeros(int(COUNT[p]), LD), np.zeros(int(COUNT[p]))
        start = 0
        for q in range(p0, p + 1):
            end = int(COUNT[q])
            _, _, c, bound = fits.get(lo, hi, q, depth)
            co[start:end], cb[start:end] = c[start:end], bound[start:end]
            start = end
        if self.mutant == "w_new_rows" and kind == "P" and p > p0:
            co[:int(COUNT[p - 1])] = 0
            cb[:int(COUNT[p - 1])] = 0
        return co, cb

    def means(self, fits, items):
        """The signed means of arrays (lo, hi, depth, p0, p, kind) -> [(mean, bound)], batched by (p, depth)."""
        m = self.mutant
        count = 99 if m == "w_99" else N_SAMPLES
        shift = 1 if m == "w_shift1" else 2
        groups = {}
        for it in items:
            k = self.key(*it)
            if ("m", k) not in self.cache:
                groups.setdefault((int(it[4]), int(it[2])), {})[k] = it
        for (p, depth), todo in groups.items():
            keys = list(todo)
            fits.ensure([(it[0], it[1], q, depth, None) for it in todo.values() for q in range(int(it[3]), p + 1)])
            step = max(1, 2 ** 18 // (int(COUNT[p]) * N_SAMPLES))
            for i in range(0, len(keys), step):
                part = keys[i:i + step]
                arr = [self.array(fits, *todo[k]) for k in part]
                lo = np.array([todo[k][0] for k in part], np.float32)
                hi = np.array([todo[k][1] for k in part], np.float32)
                _, x = sample_points(lo, hi, depth, p, count, shift, m != "w_key_nodegree")
                mean, bound = mean_reference(np.array([a[0] for a in arr], LD), np.array([a[1] for a in arr]), x, p, depth)
                for j, k in enumerate(part):
                    self.cache["m", k] = (mean[j], float(bound[j]))
        return [self.cache["m", self.key(*it)] for it in items]

    def weights(self, fits, items):
        """-> [(w, bound)] for arrays (lo, hi, depth, p0, p, kind)."""
        out = []
        for it, (mean, mb) in zip(items, self.means(fits, items)):
            k = self.key(*it)
            if ("w", k) not in self.cache:
                w, wb, tag = weight_from_mean(self.wtype, self.strength, mean, mb, self.mutant)
                self.cache["w", k] = (w, wb)
                self.seen["arrays"] += 1
                if tag:
                    self.seen[tag] += 1
                self.seen["max_degree"] = max(self.seen["max_degree"], int(it[4]))
                if it[5] == "P":
                    self.seen["appends_carried"] = max(self.seen["appends_carried"], int(it[4]) - 1 - int(it[3]))
            out.append(self.cache["w", k])
        return out
