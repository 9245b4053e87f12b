"""ProjectToSurface restated in numpy (include/hpsdf.h, "ProjectToSurface"): the loop step by step over the rows still live, one
H.query_gradient_block call per step -- that entry is pinned by its own tests (test_query_gradient_cpu.py), and every statement of the
loop (the residual, z, s, the update) is a separate float64 numpy operation, so nothing can be contracted into a fused multiply-add.
What it returns is the expected value of hpsdf_project_* bit for bit.  Also the acceptance rule of hpsdf_surface_project_vertices."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
CONVERGED, ITER_LIMIT, LEFT_ROOT, FLAT = 0, 1, 2, 3


def sum3(a, b, c, left):
    return (a + b) + c if left else a + (b + c)


def project_reference(H, blk, pts, iso=0.0, tol=1e-9, max_iter=16, unit=False, left=None):
    """-> (points [n,3], values [n], grad [n,3], iters u8 [n], status u8 [n]).  left: the reduction order of z (default: the
    process-wide one, which is also what query_gradient_block normalises with)."""
    left = bool(H.reduction_order()) if left is None else bool(left)
    x = np.array(pts, np.float64).reshape(-1, 3)
    n = len(x)
    val, grad = np.empty(n), np.empty((n, 3))
    k, status = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    live = np.arange(n)
    turns = 0
    with np.errstate(all="ignore"):
        while len(live):
            turns += 1
            assert turns <= max_iter + 1
            f, g = H.query_gradient_block(blk, x[live])
            val[live], grad[live] = f, g
            st = np.full(len(live), -1, np.int64)
            st[f == DBL_MAX] = LEFT_ROOT
            r = f - iso
            st[(st < 0) & (np.abs(r) <= tol)] = CONVERGED
            a, b, c = g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2]
            z = sum3(a, b, c, left)
            st[(st < 0) & ~(z > 0)] = FLAT
            st[(st < 0) & (k[live] == max_iter)] = ITER_LIMIT
            go = st < 0
            s = r[go] / z[go]
            rows = live[go]
            for ax in range(3):
                step = s * g[go, ax]
                x[rows, ax] = x[rows, ax] - step
            k[rows] += 1
            status[live[~go]] = st[~go]
            live = rows
        if unit:
            a, b, c = grad[:, 0] * grad[:, 0], grad[:, 1] * grad[:, 1], grad[:, 2] * grad[:, 2]
            z = sum3(a, b, c, left)
            grad = np.where((z > 0)[:, None], grad / np.sqrt(z)[:, None], grad)
    assert (status >= 0).all() and (k <= max_iter).all()
    return x, val, grad, k.astype(np.uint8), status.astype(np.uint8)


def accept_vertices(verts, projected, status, h):
    """hpsdf_surface_project_vertices' rule: vertex i becomes its projection iff status[i] == CONVERGED and |projected - vertex| <= 0.5 h
    on every axis; any other vertex stays as it was -> (verts [V,3], n_moved)."""
    verts, projected = np.asarray(verts, np.float64), np.asarray(projected, np.float64)
    half = 0.5 * np.asarray(h, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(status) == CONVERGED) & (np.abs(projected - verts) <= half).all(1)
    return np.where(ok[:, None], projected, verts), int(ok.sum())
