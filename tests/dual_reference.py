"""Restatement of hpsdf_extract_surface_dual's lattice -> mesh step, written from the text of include/hpsdf.h alone: the same ordering,
the same IEEE statements (Python floats are doubles, one rounding a statement, no fused multiply-add) and the same Jacobi.  It takes
the lattice values, the Hermite data from query_gradient_block and the lattice coordinates of surface_reference.lattice."""
import math

import numpy as np

import surface_reference as S

SWEEPS = 5  # HPSDF_DUAL_SWEEPS
CLAMPED = 4  # HPSDF_DUAL_CLAMPED
DBL_MAX = float(np.finfo(np.float64).max)


def sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


def finite(x):
    return abs(x) <= DBL_MAX  # False for NaN


def crossing_edges(vals, lo, hi, n, iso):
    """(ids, points): the crossing edges' ids 3 L + axis in increasing order and hpsdf_extract_surface's vertex on each."""
    n = [int(x) for x in n]
    N0, N1, N2 = n[0] + 1, n[1] + 1, n[2] + 1
    v = np.asarray(vals, np.float64).reshape(N2, N1, N0)
    flat = v.ravel()
    _, coords = S.lattice(lo, hi, n)
    inside = v < iso
    ids, pos = [], []
    for a in range(3):
        sl_lo, sl_hi = [slice(None)] * 3, [slice(None)] * 3
        sl_lo[2 - a], sl_hi[2 - a] = slice(0, -1), slice(1, None)
        kk, jj, ii = np.nonzero(inside[tuple(sl_lo)] != inside[tuple(sl_hi)])
        L = ii + N0 * (jj + N1 * kk)
        va, vb = flat[L], flat[L + (1, N0, N0 * N1)[a]]
        t = (iso - va) / (vb - va)
        idx = (ii, jj, kk)
        p = np.stack([coords[d][idx[d]] for d in range(3)], axis=1)
        xa, xb = coords[a][idx[a]], coords[a][idx[a] + 1]
        p[:, a] = xa + t * (xb - xa)
        ids.append(3 * L.astype(np.int64) + a)
        pos.append(p)
    ids, pos = np.concatenate(ids), np.concatenate(pos)
    order = np.argsort(ids, kind="stable")
    return ids[order], np.ascontiguousarray(pos[order])


def rotate(a, v, p, q, r):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    at = -theta if theta < 0.0 else theta
    t = 1.0 / (at + math.sqrt(theta * theta + 1.0))
    if theta < 0.0:
        t = -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        vkp, vkq = v[k][p], v[k][q]
        v[k][p] = c * vkp - s * vkq
        v[k][q] = s * vkp + c * vkq


def solve(P, F, G, iso, tau, left, cube_lo, cube_hi, sweeps=SWEEPS):
    """One cube: its crossing edges' points P, values F and gradients G in cube-local edge order -> (x, info, residual), residual being
    the largest |off-diagonal| entry over the trace after the last sweep (None when the trace is not positive)."""
    k = len(P)
    s = [0.0, 0.0, 0.0]
    for p in P:
        for a in range(3):
            s[a] = s[a] + p[a]
    m = [s[a] / float(k) for a in range(3)]
    A = [[0.0] * 3 for _ in range(3)]
    b = [0.0] * 3
    for p, f, g in zip(P, F, G):
        d = [p[a] - m[a] for a in range(3)]
        r = (iso - f) + sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], left)
        for i in range(3):
            for j in range(3):
                A[i][j] = A[i][j] + g[i] * g[j]
            b[i] = b[i] + g[i] * r
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(sweeps):
        rotate(A, V, 0, 1, 2)
        rotate(A, V, 0, 2, 1)
        rotate(A, V, 1, 2, 0)
    lam = [A[0][0], A[1][1], A[2][2]]
    trace = lam[0] + lam[1] + lam[2]
    residual = max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2])) / trace if trace > 0.0 and finite(trace) else None
    lmax = lam[0]
    if lam[1] > lmax:
        lmax = lam[1]
    if lam[2] > lmax:
        lmax = lam[2]
    x, rank = list(m), 0
    if lmax > 0.0 and finite(lmax):
        thr = tau * lmax
        for i in range(3):
            if not (lam[i] > thr and lam[i] > 0.0):
                continue
            w = sum3(V[0][i] * b[0], V[1][i] * b[1], V[2][i] * b[2], left) / lam[i]
            for a in range(3):
                x[a] = x[a] + V[a][i] * w
            rank += 1
        if not (finite(x[0]) and finite(x[1]) and finite(x[2])):
            x, rank = list(m), 0
    info = rank
    for a in range(3):
        if x[a] < cube_lo[a]:
            x[a], info = cube_lo[a], info | CLAMPED
        if x[a] > cube_hi[a]:
            x[a], info = cube_hi[a], info | CLAMPED
    return x, info, residual


def extract(H, blk, vals, lo, hi, n, iso, tau, left, sweeps=SWEEPS):
    """-> dict(verts f64 [V,3], tris u64 [T,3], info u8 [V], cubes: the mixed cubes' Q, k: their crossing-edge counts, residuals: the
    Jacobi residual of every cube with a positive trace, interior: the number of interior crossing edges)."""
    n = [int(x) for x in n]
    N0, N1 = n[0] + 1, n[1] + 1
    flat = np.asarray(vals, np.float64).ravel()
    _, coords = S.lattice(lo, hi, n)
    ids, pts = crossing_edges(vals, lo, hi, n, iso)
    if len(ids):
        F, G = H.query_gradient_block(blk, pts)
    else:
        F, G = np.zeros(0), np.zeros((0, 3))
    rec = {int(e): i for i, e in enumerate(ids)}
    P, F, G = pts.tolist(), F.tolist(), G.tolist()
    off = [0, 1, N0, N0 + 1, N0 * N1, N0 * N1 + 1, N0 * N1 + N0, N0 * N1 + N0 + 1]
    verts, info, cubes, ks, residuals = [], [], [], [], []
    vid = {}
    for Q in range(n[0] * n[1] * n[2]):
        i, j, k = Q % n[0], (Q // n[0]) % n[1], (Q // n[0]) // n[1]
        L0 = i + N0 * (j + N1 * k)
        mine = []
        for e in range(12):
            ge = 3 * (L0 + off[int(S.EDGE_CORNER[e])]) + int(S.EDGE_AXIS[e])
            if ge in rec:
                mine.append(rec[ge])
        case = sum((1 << c) for c in range(8) if flat[L0 + off[c]] < iso)
        assert (case not in (0, 255)) == bool(mine)
        if not mine:
            continue
        idx = (i, j, k)
        cube_lo = [float(coords[a][idx[a]]) for a in range(3)]
        cube_hi = [float(coords[a][idx[a] + 1]) for a in range(3)]
        x, inf, res = solve([P[r] for r in mine], [F[r] for r in mine], [G[r] for r in mine], float(iso), float(tau), left, cube_lo, cube_hi, sweeps)
        vid[Q] = len(verts)
        verts.append(x)
        info.append(inf)
        cubes.append(Q)
        ks.append(len(mine))
        if res is not None:
            residuals.append(res)
    tris = []
    for e in ids.tolist():
        L, a = e // 3, e % 3
        idx = [L % N0, (L // N0) % N1, (L // N0) // N1]
        b, c = (a + 1) % 3, (a + 2) % 3
        if not (1 <= idx[b] <= n[b] - 1 and 1 <= idx[c] <= n[c] - 1):
            continue
        q = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            id3 = list(idx)
            id3[b] += ob
            id3[c] += oc
            q.append(vid[id3[0] + n[0] * (id3[1] + n[1] * id3[2])])
        if not flat[L] < iso:
            q = [q[0], q[3], q[2], q[1]]
        tris.append((q[0], q[1], q[2]))
        tris.append((q[0], q[2], q[3]))
    return dict(verts=np.array(verts, np.float64).reshape(-1, 3), tris=np.array(tris, np.uint64).reshape(-1, 3),
                info=np.array(info, np.uint8), cubes=np.array(cubes, np.int64), k=np.array(ks, np.int64), residuals=residuals,
                interior=len(tris) // 2)
