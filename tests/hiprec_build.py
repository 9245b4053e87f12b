"""An extended-precision replay of the build loop -- the canonical round schedule of DESIGN.md section 3 -- independent of the
oracle and of the product.  It is written from Octree.cpp alone (UniformlyRefine :112-191, RunBuildThreadPool :194-309, the
decision in TickBuildThread :594-601, CreateRoot :792-801, EstimateHImprovement :804-826, EstimatePImprovement :829-856,
CornerAABB / Subdivide :1096-1128) on top of hiprec.fit_reference: every error that steers the build is a long-double fit's with
that fit's own bound, and everything the reference forms in float32 (the boxes) is reproduced bit for bit in numpy.

Notation as in hiprec.py: u = 2^-53, fl(a op b) = (a op b)(1 + d) with |d| <= u, first-order bounds times SLACK = 1 + 1e-6.
No number below was chosen by looking at a kernel's or the oracle's output.

1. The coarse tree.  CreateRoot makes node 0 = [-0.5, 0.5]^3 and subdivides it; UniformlyRefine's Inserter walks children 0..7,
   subdividing a node the first time it is met, down to depth 4: 1 + 8 + 64 + 512 + 4096 = 4681 nodes in creation order, the 4096
   depth-4 nodes queued in the order they are met with INITIAL_NODE_ERR = 100 and stored degree 0.  Subdivide appends the eight
   CornerAABBs at the end of the node array; a corner's new face is (max + min) * 0.5f in float32 (:1103, :1107).

2. A job (one queued node: cell, stored degree p, depth d, queued error E).  Nine errors, each a fit_reference "e" with its
   "e_bound":
       p_err    = the fit of degree p + 1 on the cell at depth d (:851).  The reference copies the p rows and appends only
                  rows COUNT[p] .. COUNT[p + 1] - 1 (:1012-1013, :1043); its error (:1062-1069) sums the rows of total degree
                  p + 1, all of which were just formed with the rule of order 4(p + 1) + 1 -- the from-scratch fit's error.
       h_err[i] = the from-scratch fit of degree p on CornerAABB(i) at depth d + 1 (:817-820).
   A coarse job (E == 100, :806, :831) fits degree 2 from scratch (:838-842) and no children.  Stated deviations (DESIGN.md
   section 2): a coarse job always P-refines; no P fit at degree 11 and no child fits at depth 10 (the reference computes both
   and uses neither, :600-601).
       hImp = (E - 8 max_i h_err[i]) / (7 COUNT[p])                        (:825, equation 9)
       pImp = (E - 8 p_err) / (COUNT[p + 1] - COUNT[p])                    (:854, equation 8)
       refineP = p < 11 and (d == 10 or pImp > hImp);  refineH = d < 10 and not refineP;  neither: the job is dropped (:643-655).
   Bounds.  With dE, dp, dh_i the bounds of the errors: |max_i(h_i + a_i) - max_i h_i| <= max_i |a_i|, so the exact quotients move by
       (dE + 8 max dh) / (7 COUNT[p])   and   (dE + 8 dp) / (COUNT[p + 1] - COUNT[p]).
   The float64 statements: 7.0 * COUNT and the difference of the counts are exact (small integers), 8.0 * x is exact (a power
   of two), so each of :825 and :854 rounds three times -- the reciprocal, the subtraction, the product: K_IMP = 3, u K_IMP |imp|.
       d(hImp) = ((dE + 8 max dh) / (7 COUNT[p]) + K_IMP u |hImp|) SLACK,    d(pImp) likewise.
   A decision is DECIDED if |pImp - hImp| > d(pImp) + d(hImp), or if the rule leaves no choice (coarse, d == 10, p == 11).

3. The schedule.  Stop if total < target or the queue is empty (:216); round 0 takes every coarse entry,
   later rounds the top K by (error descending, node index ascending); the results are applied in node-index order; a P sets
   degree p + 1 (a coarse one 2) and queues p_err (:253-260, :286-290); an H appends eight children of degree p at the end of the
   node array and queues each with its h_err (:262-290).  With float64 errors e~_i, |e~_i - e_i| <= b_i, a top-K selection by e~
   satisfies: every selected s has e_s + b_s >= the K-th largest of (e_i - b_i), every unselected t has e_t - b_t <= the K-th
   largest of (e_i + b_i) (order statistics are monotone in every entry).  A selection is UNDECIDED if the K-th and the
   (K + 1)-th reference errors are closer than the sum of their bounds.

4. The totals.  True total: the long-double sum of the errors of all leaves (queued or dropped), summed smallest first from
   scratch whenever it is read (n non-negative terms: relative error n 2^-64, nothing beside B); its bound is the sum of the
   errors' bounds.  Float64 total, as the reference computes it:
       T = pow(8, 4) * 100 = 409 600 (exact, :212);   P: T = fl(T + fl(new - init)) (:257);
       H: T = fl(T - init) (:272), then T = fl(T + h_err[i]) for i = 0..7 (:276).
   In exact arithmetic the statements telescope to the sum of the float64 errors of the leaves (every error is added once and
   taken away once, as the same float64 number; 100 is exact), which lies within the sum of the b_i of the true total.  Every fl
   contributes at most u |its result|:
       B = u SLACK * sum over the statements of |fl result|        (a P counts |new - init| and |T|, an H nine times |T|)
       |T - true| <= B + sum_i b_i.
   B is accumulated as the additions happen -- from the float64 results themselves where float64 errors are handed in, from the
   long-double partial sums otherwise (they differ from the float64 ones by at most B: second order, 1e-13 of B, inside SLACK).
   Round 0 alone contributes u * 4096 * ~2e5 = 9e-8: below about 1e-8 the stop rule (:216) is decided by rounding, T can end
   below the target or negative while the true total is far above it.  That is the reference's arithmetic and is reproduced, not
   corrected; so the free replay cannot decide when to stop and is told the number of rounds.  What it checks instead is that
   the stop is CONSISTENT: before every round that ran true + sum b + B >= target, and after the last one true - sum b - B <
   target or the queue is empty.

5. The rows of a built leaf.  A from-scratch fit of degree p0 (a coarse job: 2; a child of an H: the parent's degree then) forms
   rows 0 .. COUNT[p0] - 1 with the rule of order 4 p0 + 1.  Every later P to degree q appends rows COUNT[q - 1] .. COUNT[q] - 1
   formed with the rule of order 4q + 1 (:1012-1017); nothing is copied or refitted.  (COUNT[6] = 83 stops one short, so row 83 =
   (6, 0, 0) is formed by the degree-7 fit.)  check_leaf_rows compares each range with fit_reference of that degree, each row
   within that fit's "bound" (one bound for every fit mode, hiprec.py section 2).

6. Nearness weighting (Config::nearnessWeighting, :1071-1092).  replay_free and Guided take weighting = (type, strength); every
   error above is then FitPolynomial's return value, the fit's error times the weight of the array that fit produced
   (hiprec_weight.py: the sampler's definition, the long-double mean of the array the fit history of section 5 gives, the weight
   and the bound of each).  Each of a job's nine errors is weighted with its own array: p_err with the P array -- the node's copied
   rows (:847) and the appended ones, at the job's depth, sampler degree p + 1 -- and h_err[i] with child i's from-scratch array at
   depth d + 1, sampler degree p.  A coarse job weights p_err alone, with its degree-2 array; its eight other header slots belong
   to no fit and check_round requires +0.0 there.  Sections 2 to 4 run unchanged on the weighted errors and their bounds: the
   decisions, the selection, the totals, B and the stop's consistency.  Section 5 applies as it stands: weighting changes no row,
   and a weighted build's rows have the provenance of an unweighted one's -- which is what shows a stale copied row.
   WEIGHT_MUTANTS are defects of this section alone (tests/test_hiprec_weight_cpu.py shows each one rejected).

7. Fields.  The replay sees the field only through hiprec.fit_reference: `spec` is an analytic field, a mesh as data (hiprec.DataField,
   eF = 0) or either under the tree-CSG wrapper (hiprec.CsgField, eF from the old tree's Query bound) -- hiprec.py section 1 -- and
   every error keeps the bound that fit gives it.  Sections 1 to 5 do not change (tests/test_hiprec_fields_cpu.py,
   tests/test_gpu_hiprec_fields.py).
"""
import numpy as np

import hiprec as R
import hiprec_weight as W

LD, U, SLACK = R.LD, R.U, R.SLACK
COUNT = R.COUNT
INITIAL_NODE_ERR = 100.0
COARSE_DEPTH, COARSE_DEGREE = 4, 2
MAX_DEPTH, MAX_DEGREE = 10, 12
INTERIOR = R.INTERIOR
K_IMP = 3
SCHEDULE_MUTANTS = ("swap_divisors", "no8_p", "no8_h", "mean_child", "child_degree+1", "child_nl_parent", "apply_desc")
WEIGHT_MUTANTS = W.MUTANTS                                  # section 6; they change nothing in an unweighted build
MUTANTS = SCHEDULE_MUTANTS + WEIGHT_MUTANTS


# ---------------------------------------------------------------------------------------------------------------- geometry
def corner_aabb(bmin, bmax, i):
    """Octree::CornerAABB (:1096-1112) in float32."""
    lo, hi = np.array(bmin, np.float32), np.array(bmax, np.float32)
    mid = (hi + lo) * np.float32(0.5)
    for d in range(3):
        if i & (1 << d):
            lo[d] = mid[d]
        else:
            hi[d] = mid[d]
    return lo, hi


class Nodes:
    """The node array: child (-1 = none), degree, depth, float32 boxes, in creation order."""

    def __init__(self):
        self.child, self.degree, self.depth, self.bmin, self.bmax = [], [], [], [], []

    def push(self, lo, hi, depth):
        self.child.append(-1)
        self.degree.append(INTERIOR)                       # Node::Node (Node.cpp:12): BASIS_MAX_DEGREE + 1 until a basis is stored
        self.depth.append(depth)
        self.bmin.append(lo)
        self.bmax.append(hi)

    def subdivide(self, n):
        """Octree::Subdivide (:1115-1128)."""
        self.child[n] = len(self.child)
        for i in range(8):
            lo, hi = corner_aabb(self.bmin[n], self.bmax[n], i)
            self.push(lo, hi, self.depth[n] + 1)

    def arrays(self):
        return {"child": np.array(self.child, np.int64), "degree": np.array(self.degree, np.int64),
                "depth": np.array(self.depth, np.int64), "bmin": np.array(self.bmin, np.float32).reshape(-1, 3),
                "bmax": np.array(self.bmax, np.float32).reshape(-1, 3)}


def coarse_tree():
    """CreateRoot (:792-801) and UniformlyRefine's Inserter loop (:112-191), statement by statement -> (Nodes, queued node order)."""
    t = Nodes()
    t.push(np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32), 0)
    t.subdivide(0)
    parent, childno, depth, queued = [0] * COARSE_DEPTH, [0] * COARSE_DEPTH, 1, []
    while True:
        cur = t.child[parent[depth - 1]] + childno[depth - 1]
        if depth < COARSE_DEPTH:
            if t.child[cur] == -1:
                t.subdivide(cur)
                parent[depth], childno[depth] = cur, 0
                depth += 1
            elif childno[depth - 1] < 7:
                childno[depth - 1] += 1
            elif depth == 1:
                break
            else:
                depth -= 1
        else:
            t.degree[cur] = 0                                  # :173
            queued.append(cur)
            if childno[depth - 1] < 7:
                childno[depth - 1] += 1
            else:
                depth -= 1
    return t, queued


# ---------------------------------------------------------------------------------------------------------------- fits, cached
class Fits:
    """fit_reference per (cell, degree, depth[, NormalisedLengths' depth]), batched by shape and computed once.  spec: whatever
    hiprec.field_eval takes -- an analytic spec, a DataField (a mesh as data) or a CsgField; replay_free, Guided and
    check_leaf_rows hand theirs through to here and look at nothing else of it."""

    def __init__(self, spec, root, left=False):
        self.spec, self.root, self.left = spec, (tuple(root[0]), tuple(root[1])), left
        self.cache = {}
        self.computed = 0

    @staticmethod
    def key(lo, hi, degree, depth, nl=None):
        return (np.asarray(lo, np.float32).tobytes() + np.asarray(hi, np.float32).tobytes(), int(degree), int(depth),
                int(depth if nl is None else nl))

    def ensure(self, wanted):
        """wanted: iterable of (lo, hi, degree, depth, nl or None)."""
        groups = {}
        for lo, hi, p, d, nl in wanted:
            k = self.key(lo, hi, p, d, nl)
            if k not in self.cache:
                groups.setdefault(k[1:], {})[k] = (lo, hi)
        for (p, d, nl), cells in groups.items():
            keys = list(cells)
            step = max(1, 2 ** 20 // (4 * p + 1) ** 3)
            for i in range(0, len(keys), step):
                part = keys[i:i + step]
                lo = np.array([cells[k][0] for k in part], np.float32)
                hi = np.array([cells[k][1] for k in part], np.float32)
                ref = R.fit_reference(self.spec, self.root[0], self.root[1], lo, hi, p, d, self.left, nl_depth=None if nl == d else nl)
                for j, k in enumerate(part):
                    self.cache[k] = (ref["e"][j], float(ref["e_bound"][j]), ref["c"][j], ref["bound"][j])
                self.computed += len(part)

    def get(self, lo, hi, degree, depth, nl=None):
        k = self.key(lo, hi, degree, depth, nl)
        if k not in self.cache:
            self.ensure([(lo, hi, degree, depth, nl)])
        return self.cache[k]


def _job_fits(lo, hi, degree, depth, coarse, mutant):
    """The fits a job needs -> (p fit or None, list of eight child fits or None), each (lo, hi, degree, depth, nl)."""
    if coarse:
        hf = [corner_aabb(lo, hi, i) + (COARSE_DEGREE, depth + 1, None) for i in range(8)] if mutant == "w_coarse_nine" else None
        return (lo, hi, COARSE_DEGREE, depth, None), hf
    pf = (lo, hi, degree + 1, depth, None) if degree < MAX_DEGREE - 1 else None
    hf = None
    if depth < MAX_DEPTH:
        hd = degree + 1 if mutant == "child_degree+1" else degree
        nl = depth if mutant == "child_nl_parent" else None
        hf = [corner_aabb(lo, hi, i) + (hd, depth + 1, nl) for i in range(8)]
    return pf, hf


def job_errors(fits, jobs, mutant=None, weighting=None):
    """jobs: [(lo, hi, degree, depth, coarse, p0)] -> per job (p, h): p = (e, bound) or None, h = [(e, bound)] * 8 or None.  With
    a weighting (a W.Weighting) every error is its fit's times the weight of its own array (section 6); p0 is the degree of the
    from-scratch fit that began the node's array (section 5), which says where a P array's rows come from."""
    need = [_job_fits(*j[:5], mutant) for j in jobs]
    fits.ensure([f for pf, hf in need for f in ([pf] if pf else []) + (hf or [])])
    out = []
    for pf, hf in need:
        out.append((fits.get(*pf)[:2] if pf else None, [fits.get(*f)[:2] for f in hf] if hf else None))
    if weighting is None:
        return out
    items, where = [], []
    for n, ((lo, hi, degree, depth, coarse, p0), (pf, hf)) in enumerate(zip(jobs, need)):
        if pf:
            items.append((lo, hi, depth, COARSE_DEGREE, COARSE_DEGREE, "C") if coarse else (lo, hi, depth, p0, degree + 1, "P"))
            where.append((n, -1))
        for i, f in enumerate(hf or []):
            own = (f[0], f[1], f[3], f[2], f[2], "H")
            items.append((lo, hi, depth, p0, degree, "H") if mutant == "w_child_parent" and not coarse else own)
            where.append((n, i))
    for (n, i), (w, wb) in zip(where, weighting.weights(fits, items)):
        p, h = out[n]
        if i < 0:
            out[n] = (W.weighted_error(p[0], p[1], w, wb), h)
        else:
            h[i] = W.weighted_error(h[i][0], h[i][1], w, wb)
    return out


def decide(err, err_b, p, h, degree, depth, coarse, mutant=None):
    """Section 2 -> dict(action 'P' | 'H' | 'D', decided, margin = |pImp - hImp| / (the two bounds), or inf where the rule leaves
    no choice)."""
    forced = None
    if coarse:
        forced = "P"
    elif depth >= MAX_DEPTH:
        forced = "P" if degree < MAX_DEGREE - 1 else "D"
    elif degree >= MAX_DEGREE - 1:
        forced = "H"
    if forced:
        return {"action": forced, "decided": True, "margin": np.inf}
    ch, cp = LD(7 * int(COUNT[degree])), LD(int(COUNT[degree + 1] - COUNT[degree]))
    if mutant == "swap_divisors":
        ch, cp = cp, ch
    he = [e for e, _ in h]
    m = sum(he) / 8 if mutant == "mean_child" else max(he)
    mb = max(b for _, b in h)
    h_imp = (err - (1 if mutant == "no8_h" else 8) * m) / ch
    p_imp = (err - (1 if mutant == "no8_p" else 8) * p[0]) / cp
    h_b = ((err_b + 8 * mb) / float(ch) + K_IMP * U * float(abs(h_imp))) * SLACK
    p_b = ((err_b + 8 * p[1]) / float(cp) + K_IMP * U * float(abs(p_imp))) * SLACK
    gap = float(abs(p_imp - h_imp))
    return {"action": "P" if p_imp > h_imp else "H", "decided": gap > h_b + p_b, "margin": gap / (h_b + p_b),
            "p_imp": p_imp, "h_imp": h_imp}


def decide_f64(err, hdr, degree, depth, coarse):
    """:594-601 with :825 and :854 in float64, statement by statement, from a job's nine float64 errors."""
    f = np.float64
    err = f(err)
    if coarse:
        return "P"
    h_imp = p_imp = f(0.0)
    if depth < MAX_DEPTH:
        mx = f(0.0)
        for i in range(8):
            mx = max(mx, f(hdr[1 + i]))
        h_imp = (f(1.0) / (f(7.0) * f(int(COUNT[degree])))) * (err - f(8.0) * mx)
    if degree < MAX_DEGREE - 1:
        p_imp = (f(1.0) / f(int(COUNT[degree + 1] - COUNT[degree]))) * (err - f(8.0) * f(hdr[0]))
    refine_p = degree < MAX_DEGREE - 1 and (depth == MAX_DEPTH or p_imp > h_imp)
    return "P" if refine_p else "H" if depth < MAX_DEPTH else "D"


# ---------------------------------------------------------------------------------------------------------------- totals
class Totals:
    """Section 4.  p() and h() take the long-double errors and, where known, the float64 ones (numpy float64 scalars)."""

    def __init__(self, with_f64):
        self.f64 = np.float64(8.0) ** 4 * np.float64(INITIAL_NODE_ERR) if with_f64 else None      # :212
        self.run = LD(4096) * LD(INITIAL_NODE_ERR)                                                 # the same statements in long double
        self.B = 0.0

    def _add(self, v, v64):
        self.run = self.run + v
        if v64 is None:
            self.B += U * SLACK * float(abs(self.run))
        else:
            self.f64 = self.f64 + v64
            self.B += U * SLACK * float(abs(self.f64))

    def p(self, init, new, init64=None, new64=None):                                              # :257
        if new64 is None:
            self.B += U * SLACK * float(abs(new - init))
            self._add(new - init, None)
        else:
            t = np.float64(new64) - np.float64(init64)
            self.B += U * SLACK * float(abs(t))
            self._add(new - init, t)

    def h(self, init, news, init64=None, news64=None):                                            # :272, :276
        self._add(-init, None if news64 is None else -np.float64(init64))
        for i in range(8):
            self._add(news[i], None if news64 is None else np.float64(news64[i]))


def true_total(errs):
    """The long-double sum of (error, bound) pairs, smallest first -> (sum, sum of the bounds)."""
    v = np.sort(np.array([e for e, _ in errs], LD))
    return (v.sum() if len(v) else LD(0)), float(sum(b for _, b in errs))


# ---------------------------------------------------------------------------------------------------------------- the tree under replay
class _State:
    def __init__(self, spec, root, left, fits, weighting=None, mutant=None):
        self.fits = fits if fits is not None else Fits(spec, root, left)
        self.weighting = weighting if weighting is None or isinstance(weighting, W.Weighting) else W.Weighting(*weighting, mutant=mutant)
        self.t, coarse = coarse_tree()
        self.queue = {n: (LD(INITIAL_NODE_ERR), 0.0) for n in coarse}     # node -> (reference error, bound)
        self.dropped = {}
        self.hist = {}                                                    # leaf -> [p0, [degrees appended since]]
        self.counts = {"rounds": 0, "jobs": 0, "p_refines": 0, "h_refines": 0, "dropped": 0}
        self.job_log = {}                                                 # (stored degree, depth, coarse) -> jobs applied

    def job_tuple(self, n, coarse):
        return (self.t.bmin[n], self.t.bmax[n], self.t.degree[n], self.t.depth[n], coarse, COARSE_DEGREE if coarse else self.hist[n][0])

    def apply(self, n, action, coarse, p, h):
        """One result (:253-290) on the tree and the queue; the caller moves the totals."""
        t = self.t
        self.counts["jobs"] += 1
        k = (int(t.degree[n]), int(t.depth[n]), bool(coarse))
        self.job_log[k] = self.job_log.get(k, 0) + 1
        old = self.queue.pop(n)
        if action == "P":
            if coarse:
                t.degree[n] = COARSE_DEGREE
                self.hist[n] = [COARSE_DEGREE, []]
            else:
                t.degree[n] += 1
                self.hist[n][1].append(t.degree[n])
            self.queue[n] = p
            self.counts["p_refines"] += 1
        elif action == "H":
            deg = t.degree[n]
            t.degree[n] = INTERIOR
            self.hist.pop(n)
            t.subdivide(n)
            for i in range(8):
                c = t.child[n] + i
                t.degree[c] = deg
                self.hist[c] = [deg, []]
                self.queue[c] = h[i]
            self.counts["h_refines"] += 1
        else:
            self.dropped[n] = old
            self.counts["dropped"] += 1

    def leaves_total(self):
        return true_total(list(self.queue.values()) + list(self.dropped.values()))

    def result(self):
        out = self.t.arrays()
        out.update(history={n: (p0, tuple(app)) for n, (p0, app) in self.hist.items()}, counts=dict(self.counts), fits=self.fits,
                   weighting=self.weighting, job_log=dict(self.job_log))
        return out


def replay_free(spec, root, target, K, rounds, left=False, mutant=None, fits=None, weighting=None):
    """Grow the tree from long-double errors alone for exactly `rounds` rounds (section 4: the stop itself is not decidable) ->
    dict(child, degree, depth, bmin, bmax, history, counts, job_log, undecided_decisions, undecided_selections, min_margin,
    stop_consistent, true_total, true_bound, B, fits, weighting).  weighting: None, (type, strength) or a W.Weighting (its cache
    of weights is then shared): every error below is the weighted one (section 6)."""
    s = _State(spec, root, left, fits, weighting, mutant)
    tot = Totals(False)
    undecided_d = undecided_s = 0
    min_margin, consistent = np.inf, True
    for r in range(rounds):
        tt, tb = s.leaves_total()
        if not s.queue or float(tt) + tb + tot.B < target:
            consistent = False                                   # the product went on where the true total had to be below target
        order = sorted(s.queue, key=lambda n: (-s.queue[n][0], n))
        take = order if r == 0 else order[:K]
        if len(order) > len(take):
            a, b = s.queue[order[len(take) - 1]], s.queue[order[len(take)]]
            if float(a[0] - b[0]) <= a[1] + b[1]:
                undecided_s += 1
        take = sorted(take, reverse=(mutant == "apply_desc"))
        coarse = r == 0
        errs = job_errors(s.fits, [s.job_tuple(n, coarse) for n in take], mutant, s.weighting)
        for n, (p, h) in zip(take, errs):
            e, eb = s.queue[n]
            d = decide(e, eb, p, h, s.t.degree[n], s.t.depth[n], coarse, mutant)
            undecided_d += not d["decided"]
            min_margin = min(min_margin, d["margin"])
            if d["action"] == "P":
                tot.p(e, p[0])
            elif d["action"] == "H":
                tot.h(e, [x[0] for x in h])
            s.apply(n, d["action"], coarse, p, h)
        s.counts["rounds"] += 1
    tt, tb = s.leaves_total()
    if s.queue and not float(tt) - tb - tot.B < target:
        consistent = False                                       # the product stopped where the true total was surely not below
    out = s.result()
    out.update(undecided_decisions=undecided_d, undecided_selections=undecided_s, min_margin=min_margin, stop_consistent=consistent,
               true_total=tt, true_bound=tb, B=tot.B, queue_left=len(s.queue))
    return out


# ---------------------------------------------------------------------------------------------------------------- the guided form
class Guided:
    """check_round for the stepwise API: follows the product's selections round by round and checks everything else."""

    def __init__(self, spec, root, target, K, left=False, mutant=None, fits=None, weighting=None):
        self.s = _State(spec, root, left, fits, weighting, mutant)
        self.target, self.K, self.mutant = target, K, mutant
        self.tot = Totals(True)
        self.q64 = {n: np.float64(INITIAL_NODE_ERR) for n in self.s.queue}      # the float64 errors the product queued
        self.worst = {"job_error": 0.0, "selection_ties": 0, "undecided": 0, "min_margin": np.inf}
        self.small_rounds = 0                                                    # rounds with fewer than K queued entries

    def check_round(self, jobs, headers):
        """jobs: [(node index, bmin, bmax, err, degree, depth, coarse)] as Build.jobs lists them; headers: [n, 9] float64, a
        job's p_err and eight h_err.  Raises AssertionError on the first check that fails."""
        s, r = self.s, self.s.counts["rounds"]
        headers = np.asarray(headers, np.float64).reshape(len(jobs), 9)
        assert not self.tot.f64 < self.target and s.queue, "a round was opened although total < target or the queue was empty (:216)"
        coarse = r == 0
        want = len(s.queue) if coarse else min(self.K, len(s.queue))
        assert len(jobs) == want, "round %d selects %d of %d queued entries, not %d" % (r, len(jobs), len(s.queue), want)
        self.small_rounds += (not coarse) and len(s.queue) < self.K
        sel = [int(j[0]) for j in jobs]
        assert sel == sorted(set(sel)), "round %d: the jobs are not in node-index order" % r
        for n, lo, hi, err, degree, depth, jc in jobs:
            assert n in s.queue, "round %d: node %d is not queued" % (r, n)
            assert np.array_equal(np.asarray(lo, np.float32), s.t.bmin[n]) and np.array_equal(np.asarray(hi, np.float32), s.t.bmax[n]), \
                "round %d: node %d's box" % (r, n)
            assert (int(degree), int(depth), bool(jc)) == (s.t.degree[n], s.t.depth[n], coarse), "round %d: node %d's degree, depth or coarse flag" % (r, n)
            assert np.float64(err).tobytes() == self.q64[n].tobytes(), "round %d: node %d's queued error is not the one its fit returned" % (r, n)
        # selection (section 3)
        if len(s.queue) > want:
            e = np.array([float(v[0]) for v in s.queue.values()])
            b = np.array([v[1] for v in s.queue.values()])
            lo_k, hi_k = np.sort(e - b)[-want], np.sort(e + b)[-want]
            chosen = set(sel)
            for n, (ev, bv) in s.queue.items():
                if n in chosen:
                    assert float(ev) + bv >= lo_k, "round %d: node %d selected below the K-th error by more than the bounds" % (r, n)
                else:
                    assert float(ev) - bv <= hi_k, "round %d: node %d left out above the K-th error by more than the bounds" % (r, n)
            order = sorted(s.queue, key=lambda n: (-s.queue[n][0], n))
            a, c = s.queue[order[want - 1]], s.queue[order[want]]
            self.worst["selection_ties"] += float(a[0] - c[0]) <= a[1] + c[1]
        # errors and decisions (section 2)
        errs = job_errors(s.fits, [s.job_tuple(n, coarse) for n in sel], self.mutant, s.weighting)
        acts = []
        for (n, _, _, err, degree, depth, _), hdr, (p, h) in zip(jobs, headers, errs):
            live = ([(hdr[0], p)] if p else []) + ([(hdr[1 + i], h[i]) for i in range(8)] if h else [])
            for got, (ev, bv) in live:
                ratio = float(abs(LD(got) - ev)) / bv if bv > 0 else (0.0 if LD(got) == ev else np.inf)
                self.worst["job_error"] = max(self.worst["job_error"], ratio)
                assert ratio <= 1, "round %d: node %d: an error is %.3g bounds from the reference" % (r, n, ratio)
            if s.weighting is not None and coarse and h is None:
                # section 6: a coarse job's eight other slots belong to no fit; nothing may have been weighted into them
                assert all(np.float64(v).tobytes() == np.float64(0.0).tobytes() for v in hdr[1:9]), \
                    "round %d: node %d: a header slot that belongs to no fit is not +0.0" % (r, n)
            ev, eb = s.queue[n]
            d = decide(ev, eb, p, h, s.t.degree[n], s.t.depth[n], coarse, self.mutant)
            act = decide_f64(err, hdr, s.t.degree[n], s.t.depth[n], coarse)
            self.worst["undecided"] += not d["decided"]
            self.worst["min_margin"] = min(self.worst["min_margin"], d["margin"])
            assert not d["decided"] or d["action"] == act, \
                "round %d: node %d: the decision is %s by %.3g bounds, float64 takes %s" % (r, n, d["action"], d["margin"], act)
            acts.append(act)
        # apply in node-index order (the product's own order; its tree is compared at the next round and at the end)
        for (n, _, _, err, _, _, _), hdr, (p, h), act in zip(jobs, headers, errs, acts):
            ev = s.queue[n][0]
            if act == "P":
                self.tot.p(ev, p[0], err, hdr[0])
                self.q64[n] = np.float64(hdr[0])
            elif act == "H":
                self.tot.h(ev, [x[0] for x in h], err, hdr[1:9])
                del self.q64[n]
            s.apply(n, act, coarse, p, h)
            if act == "H":
                for i in range(8):
                    self.q64[s.t.child[n] + i] = np.float64(hdr[1 + i])
        s.counts["rounds"] += 1

    def finish(self, block, stats):
        """After the last round: the product's tree is this tree, its statistics these counts, its total_error the restated
        float64 total bit for bit and within B + sum of bounds of the true total -> dict of what was observed."""
        s = self.s
        assert self.tot.f64 < self.target or not s.queue, "the build stopped although total >= target and entries were queued (:216)"
        same_tree(block, s.t.arrays())
        for k, v in s.counts.items():
            assert stats[k] == v, (k, stats[k], v)
        assert np.float64(stats["total_error"]).tobytes() == self.tot.f64.tobytes(), (stats["total_error"], float(self.tot.f64))
        tt, tb = s.leaves_total()
        drift = float(abs(LD(self.tot.f64) - tt))
        assert drift <= self.tot.B + tb, (drift, self.tot.B, tb)
        out = dict(self.worst)
        out.update(drift=drift, B=self.tot.B, drift_over_B=drift / self.tot.B, true_total=tt, true_bound=tb, f64_total=float(self.tot.f64),
                   small_rounds=self.small_rounds, history=s.result()["history"], counts=dict(s.counts), weighting=s.weighting,
                   job_log=dict(s.job_log))
        return out


def job_list(jobs):
    """Build.jobs' ctypes array -> the tuples check_round takes."""
    return [(int(j.node_idx), np.array(j.aabb_min[:], np.float32), np.array(j.aabb_max[:], np.float32), np.float64(j.err),
             int(j.degree), int(j.depth), int(j.coarse)) for j in jobs]


def same_tree(block, tree):
    """A MemoryBlock's topology against a replay's: childIdx, degree, depth and the boxes, node by node."""
    b = block if isinstance(block, R.Block) else R.Block(block)
    assert len(b.child) == len(tree["child"]), (len(b.child), len(tree["child"]))
    assert np.array_equal(b.child, tree["child"].astype(np.uint64)), "childIdx differs first at node %d" % int(
        np.nonzero(b.child != tree["child"].astype(np.uint64))[0][0])
    assert np.array_equal(b.degree, tree["degree"]), "degree differs first at node %d" % int(np.nonzero(b.degree != tree["degree"])[0][0])
    assert np.array_equal(b.depth, tree["depth"])
    assert np.array_equal(b.bmin, tree["bmin"]) and np.array_equal(b.bmax, tree["bmax"])


# ---------------------------------------------------------------------------------------------------------------- leaf rows
def _rows_ratio(fits, lo, hi, depth, rows, p0, p, final_fit=False):
    """max |row - reference| / bound with rows < COUNT[p0] from the degree-p0 fit and rows COUNT[q - 1] .. COUNT[q] - 1 from the
    degree-q fit, q = p0 + 1 .. p (final_fit: the mutant that takes every row from the degree-p fit)."""
    worst, start = 0.0, 0
    for q in range(p0, p + 1):
        end = int(COUNT[q])
        _, _, c, bound = fits.get(lo, hi, p if final_fit else q, depth)
        diff = np.abs(rows[start:end].astype(LD) - c[start:end]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound[start:end] > 0, diff / bound[start:end], np.where(diff > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
        start = end
    return worst


def check_leaf_rows(block, spec, history=None, left=False, fits=None, leaves=None, final_fit=False):
    """Every leaf's rows (or those of `leaves`) against the fits that formed them (section 5) -> dict(worst, p0 = {leaf: p0},
    chains = the longest run of appended degrees).  With the replay's history p0 is known; without it some p0 in 2..p must fit, and
    the one that does is reported."""
    b = block if isinstance(block, R.Block) else R.Block(block)
    fits = fits if fits is not None else Fits(spec, (b.root_min, b.root_max), left)
    lv = b.leaves() if leaves is None else np.asarray(leaves)
    if history is not None:
        assert set(int(n) for n in b.leaves()) == set(history), "the history's leaves are not the block's"
        want = []
        for n in lv:
            p0, app = history[int(n)]
            assert p0 + len(app) == b.degree[n] and list(app) == list(range(p0 + 1, int(b.degree[n]) + 1)), (int(n), p0, app)
            q = [int(b.degree[n])] if final_fit else range(p0, int(b.degree[n]) + 1)
            want += [(b.bmin[n], b.bmax[n], k, int(b.depth[n]), None) for k in q]
        fits.ensure(want)
    worst, found, chain = 0.0, {}, 0
    for n in lv:
        n = int(n)
        p, d = int(b.degree[n]), int(b.depth[n])
        rows = b.coeffs[b.start[n]:b.start[n] + int(COUNT[p])]
        if history is not None:
            ratio = _rows_ratio(fits, b.bmin[n], b.bmax[n], d, rows, history[n][0], p, final_fit)
            found[n] = history[n][0]
        else:
            fits.ensure([(b.bmin[n], b.bmax[n], q, d, None) for q in range(2, p + 1)])
            tried = {p0: _rows_ratio(fits, b.bmin[n], b.bmax[n], d, rows, p0, p) for p0 in range(2, p + 1)}
            ok = [p0 for p0, v in tried.items() if v <= 1]
            assert ok, "leaf %d (degree %d, depth %d): no p0 in 2..%d explains its rows, best %.3g bounds" % (n, p, d, p, min(tried.values()))
            found[n], ratio = ok[0], tried[ok[0]]
        chain = max(chain, p - found[n])
        worst = max(worst, ratio)
    return {"worst": worst, "p0": found, "chain": chain}
