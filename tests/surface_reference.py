"""numpy restatement of hpsdf_extract_surface's lattice -> mesh step (include/hpsdf.h): the same ordering and the same IEEE
arithmetic, from the lattice values and the case table of hpsdf_surface_case_table."""
import numpy as np

# cube-local edge -> (lower corner, axis); corners c = dx + 2 dy + 4 dz
EDGE_CORNER = np.array([0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3])
EDGE_AXIS = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2])
EDGE_ENDS = [(int(c), int(c) | (1 << int(a))) for c, a in zip(EDGE_CORNER, EDGE_AXIS)]


def lattice(lo, hi, n):
    """(h, coords): h[a] = (hi - lo) / n, coords[a][i] = lo + (f64)i * h (two roundings)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    h = (hi - lo) / np.asarray(n, np.float64)
    return h, [lo[a] + np.arange(int(n[a]) + 1, dtype=np.float64) * h[a] for a in range(3)]


def lattice_points(lo, hi, n):
    """Every lattice point, L order (x fastest), as an (N, 3) array."""
    _, c = lattice(lo, hi, n)
    z, y, x = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def extract(vals, lo, hi, n, iso, table):
    """vals: (n2+1, n1+1, n0+1) lattice values; table: int8 [256, 16].  -> (verts f64 [V,3], tris u64 [T,3])."""
    n = [int(x) for x in n]
    N0, N1, N2 = n[0] + 1, n[1] + 1, n[2] + 1
    v = np.asarray(vals, np.float64).reshape(N2, N1, N0)
    flat = v.ravel()
    h, coords = lattice(lo, hi, n)
    inside = v < iso
    # crossing edges: edge id 3 L + axis, L of the lower point
    ids, pos = [], []
    for a in range(3):
        sl_lo = [slice(None)] * 3
        sl_hi = [slice(None)] * 3
        ax = 2 - a  # array axis of lattice axis a
        sl_lo[ax] = slice(0, -1)
        sl_hi[ax] = slice(1, None)
        cross = inside[tuple(sl_lo)] != inside[tuple(sl_hi)]
        kk, jj, ii = np.nonzero(cross)
        L = ii + N0 * (jj + N1 * kk)
        stride = (1, N0, N0 * N1)[a]
        va, vb = flat[L], flat[L + stride]
        t = (iso - va) / (vb - va)
        idx = (ii, jj, kk)
        p = np.stack([coords[d][idx[d]] for d in range(3)], axis=1)
        xa = coords[a][idx[a]]
        xb = coords[a][idx[a] + 1]
        p[:, a] = xa + t * (xb - xa)
        ids.append(3 * L.astype(np.int64) + a)
        pos.append(p)
    ids = np.concatenate(ids)
    pos = np.concatenate(pos)
    order = np.argsort(ids, kind="stable")
    ids, verts = ids[order], pos[order]
    # cubes in Q order, then their case rows
    cs = np.zeros((n[2], n[1], n[0]), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cs |= inside[dz:dz + n[2], dy:dy + n[1], dx:dx + n[0]].astype(np.int64) << c
    cs = cs.ravel()
    tab = np.asarray(table, np.int64).reshape(256, 16)
    cnt = (tab >= 0).sum(axis=1) // 3
    q = np.arange(len(cs))
    qi, qr = q % n[0], q // n[0]
    qj, qk = qr % n[1], qr // n[1]
    L0 = qi + N0 * (qj + N1 * qk)
    sel = np.nonzero(cnt[cs][:, None] > np.arange(5)[None, :])  # (cube, slot), cube-major
    cube, slot = sel
    tris = np.zeros((len(cube), 3), np.uint64)
    off = np.array([0, 1, N0, N0 + 1, N0 * N1, N0 * N1 + 1, N0 * N1 + N0, N0 * N1 + N0 + 1], np.int64)
    for m in range(3):
        le = tab[cs[cube], 3 * slot + m]
        ge = 3 * (L0[cube] + off[EDGE_CORNER[le]]) + EDGE_AXIS[le]
        vid = np.searchsorted(ids, ge)
        assert np.array_equal(ids[vid], ge), "a triangle names an edge that does not cross"
        tris[:, m] = vid.astype(np.uint64)
    return verts, tris


def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def unmatched_edges(tris):
    """Directed edges whose reverse is not present exactly once (and edges present more than once)."""
    from collections import Counter
    e = Counter(map(tuple, directed_edges(tris).tolist()))
    return [k for k, c in e.items() if c != 1 or e.get((k[1], k[0]), 0) != 1]


def euler_characteristic(verts, tris):
    t = np.asarray(tris, np.int64)
    und = np.sort(directed_edges(t), axis=1)
    E = len(np.unique(und, axis=0))
    V = len(np.unique(t))
    return V - E + len(t)


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def components(tris):
    """Connected components of the triangles (through shared vertices)."""
    t = np.asarray(tris, np.int64)
    parent = np.arange(int(t.max()) + 1 if len(t) else 0)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in t:
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[ru] = rw
    return len({find(x) for x in np.unique(t)})
