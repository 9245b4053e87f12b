"""CastRays restated in numpy (include/hpsdf.h, "CastRays"): the five steps written out per ray as the header states them, every
statement one float64 operation on numpy scalars, so nothing can be contracted into a fused multiply-add.  The field is evaluated only
through H.query_gradient_block -- that entry is pinned by its own tests (test_query_gradient_cpu.py) -- and the leaf boxes come from
hiprec.Block (its descent and the serialised f32 boxes, which are exact dyadics).  Each ray is a generator that asks for one
evaluation or one descent at a time; the driver answers all live rays' requests in one call per turn.  What cast_reference returns is
the expected output of hpsdf_cast_rays_* bit for bit."""
import numpy as np

import hiprec as R

F64 = np.float64
DBL_MAX = np.finfo(np.float64).max
NAN = F64(np.nan)
HIT, MISS, UNCONVERGED, CELL_LIMIT, INVALID = 0, 1, 2, 3, 4


def sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


def below(v):
    """the largest double less than v"""
    return np.nextafter(F64(v), F64(-np.inf))


def point_at(o, d, t):
    """x(t)_a = o_a + t d_a: one multiply, one add"""
    out = []
    for a in range(3):
        m = t * d[a]
        out.append(o[a] + m)
    return out


def _row(status, t=NAN, x=(NAN, NAN, NAN), f=F64(DBL_MAX), g=(NAN, NAN, NAN), evals=0, cells=0):
    return status, t, tuple(x), f, tuple(g), min(evals, 65535), min(cells, 65535)


def _refine(o, d, a, b, ra, cur, f, g, iso, tol, max_iter, left, evals, cells):
    """step 5 on the bracket [a, b]; (f, g) is QueryGradient at b"""
    fb, gb = f, g
    c, rc, sc = b, cur, sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], left)
    k, halved = 0, True
    while True:
        q = rc / sc
        tn = c - q
        if halved and tn > a and tn < b:
            m = tn
        else:
            w = b - a
            m = a + F64(0.5) * w
        if not (m > a and m < b) or k == max_iter:
            return _row(UNCONVERGED, b, point_at(o, d, b), fb, gb, evals, cells)
        x = point_at(o, d, m)
        f, g = yield ("eval", x)
        evals += 1
        if f == DBL_MAX:
            return _row(UNCONVERGED, b, point_at(o, d, b), fb, gb, evals, cells)
        rm = f - iso
        if abs(rm) <= tol:
            return _row(HIT, m, x, f, g, evals, cells)
        w = b - a
        if (rm < 0) == (ra < 0):
            a, ra = m, rm
        else:
            b, fb, gb = m, f, g
        c, rc, sc = m, rm, sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], left)
        halved = (b - a) <= F64(0.5) * w
        k += 1


def _ray(o, d, t_max, centre, inv, iso, tol, max_iter, max_cells, left):
    """one ray: yields ("eval", x) -> (f, g) and ("locate", pu) -> (lo, hi, degree); returns its row"""
    # 1 validity
    if not (np.isfinite(o).all() and np.isfinite(d).all()) or (d == 0).all() or not (t_max >= 0):
        return _row(INVALID)
    # 2 clip
    ou = [(o[a] - centre[a]) * inv[a] for a in range(3)]
    du = [d[a] * inv[a] for a in range(3)]
    t0, t1 = F64(0.0), t_max
    for a in range(3):
        if du[a] == 0:
            if not (ou[a] >= -0.5 and ou[a] <= 0.5):
                return _row(MISS)
            continue
        tl = (F64(-0.5) - ou[a]) / du[a]
        th = (F64(0.5) - ou[a]) / du[a]
        tin, tout = (tl, th) if du[a] > 0 else (th, tl)
        if tin > t0:
            t0 = tin
        if tout < t1:
            t1 = tout
    if not (t0 <= t1):
        return _row(MISS)
    # 3 first sample
    evals = 0
    x = point_at(o, d, t0)
    f, g = yield ("eval", x)
    evals += 1
    if f == DBL_MAX:
        return _row(MISS, evals=evals)
    prev, t_prev = f - iso, t0
    if abs(prev) <= tol:
        return _row(HIT, t0, x, f, g, evals, 0)
    # 4 walk
    pu = []
    for a in range(3):
        m = t0 * du[a]
        pu.append(min(max(ou[a] + m, F64(-0.5)), F64(0.5)))
    lo, hi, p = yield ("locate", pu)
    cells, t = 1, t0
    while True:
        e, tb = -1, None
        for a in range(3):
            if du[a] == 0:
                continue
            face = hi[a] if du[a] > 0 else lo[a]
            ta = (face - ou[a]) / du[a]
            if e < 0 or ta < tb:
                tb, e = ta, a
        if e < 0:
            tb = t1
        else:
            if not (tb >= t):
                tb = t
            if not (tb <= t1):
                tb = t1
        if tb > t:
            S = max(1, p)
            for j in range(1, S + 1):
                if j == S:
                    tj = tb
                else:
                    w = F64(j) / F64(S)
                    m = (tb - t) * w
                    tj = t + m
                x = point_at(o, d, tj)
                f, g = yield ("eval", x)
                evals += 1
                if f == DBL_MAX:
                    return _row(MISS, evals=evals, cells=cells)
                cur = f - iso
                if abs(cur) <= tol:
                    return _row(HIT, tj, x, f, g, evals, cells)
                if (prev < 0) != (cur < 0):
                    return (yield from _refine(o, d, t_prev, tj, prev, cur, f, g, iso, tol, max_iter, left, evals, cells))
                prev, t_prev = cur, tj
        if tb >= t1:
            return _row(MISS, evals=evals, cells=cells)
        if (hi[e] >= 0.5) if du[e] > 0 else (lo[e] <= -0.5):
            return _row(MISS, evals=evals, cells=cells)
        if cells == max_cells:
            return _row(CELL_LIMIT, evals=evals, cells=cells)
        pu = []
        for a in range(3):
            if a == e:
                pu.append(hi[a] if du[a] > 0 else below(lo[a]))
                continue
            m = tb * du[a]
            q = ou[a] + m
            top = below(hi[a])
            if not (q >= lo[a]):
                q = lo[a]
            if not (q <= top):
                q = top
            pu.append(q)
        lo, hi, p = yield ("locate", pu)
        cells += 1
        t = tb


def cast_reference(H, blk, origins, dirs, t_max, iso=0.0, tol=1e-9, max_iter=32, max_cells=4096, unit=False, left=None):
    """-> (status u8 [n], t [n], points [n,3], values [n], grad [n,3], evals u16 [n], cells u16 [n]).  left: the reduction order of
    s(t) (default: the process-wide one, which is also what query_gradient_block normalises with)."""
    left = bool(H.reduction_order()) if left is None else bool(left)
    raw = bytes(blk)
    B = R.Block(raw)
    o = np.array(origins, np.float64).reshape(-1, 3)
    d = np.array(dirs, np.float64).reshape(-1, 3)
    n = len(o)
    tm = np.array(np.broadcast_to(np.asarray(t_max, np.float64), (n,)))
    centre = ((B.root_min + B.root_max) / np.float32(2.0)).astype(np.float64)
    inv = (np.float32(1.0) / (B.root_max - B.root_min)).astype(np.float64)
    iso, tol = F64(iso), F64(tol)
    rows, gens, want = [None] * n, {}, {}

    def advance(i, answer):
        try:
            want[i] = gens[i].send(answer)
        except StopIteration as stop:
            rows[i] = stop.value
            del gens[i]
            want.pop(i, None)

    with np.errstate(all="ignore"):
        for i in range(n):
            gens[i] = _ray(o[i], d[i], tm[i], centre, inv, iso, tol, int(max_iter), int(max_cells), left)
            advance(i, None)
        while gens:
            ev = [i for i in gens if want[i][0] == "eval"]
            lc = [i for i in gens if want[i][0] == "locate"]
            if ev:
                f, g = H.query_gradient_block(raw, np.array([want[i][1] for i in ev], np.float64))
                for j, i in enumerate(ev):
                    advance(i, (f[j], tuple(g[j])))
            if lc:
                leaf = B.descend(np.array([want[i][1] for i in lc], np.float64))
                for j, i in enumerate(lc):
                    m = leaf[j]
                    advance(i, (B.bmin[m].astype(np.float64), B.bmax[m].astype(np.float64), int(B.degree[m])))
        status = np.array([r[0] for r in rows], np.uint8)
        t = np.array([r[1] for r in rows], np.float64).reshape(n)
        x = np.array([r[2] for r in rows], np.float64).reshape(n, 3)
        val = np.array([r[3] for r in rows], np.float64).reshape(n)
        grad = np.array([r[4] for r in rows], np.float64).reshape(n, 3)
        if unit:
            a, b, c = grad[:, 0] * grad[:, 0], grad[:, 1] * grad[:, 1], grad[:, 2] * grad[:, 2]
            z = sum3(a, b, c, left)
            grad = np.where((z > 0)[:, None], grad / np.sqrt(z)[:, None], grad)
    evals = np.array([r[5] for r in rows], np.uint16).reshape(n)
    cells = np.array([r[6] for r in rows], np.uint16).reshape(n)
    return status, t, x, val, grad, evals, cells
