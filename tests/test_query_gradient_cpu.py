"""QueryGradient without a device: hpsdf_query_true_gradient_block (the statements of the kernels on the calling thread) against the
long-double reference of tests/hiprec_gradient.py and its derived bound, the reference against mpmath, mutants the bound rejects,
the argument checks, the normalisation, an orientation-and-scale check on a built sphere, and save_obj's normals."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

import hiprec as R
import hiprec_gradient as G
from helpers import edge_points, synthetic_block
from test_hiprec_cpu import ROOTS, _with_root, query_blocks

DBL_MAX = np.finfo(np.float64).max


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def gradient_blocks(rng):
    """query_blocks (every degree 0..12, depths to 10, the unit root and [-0.25, 5]^3) and one block on an anisotropic root."""
    return query_blocks(rng) + [("aniso", _with_root(synthetic_block(rng, [3, 5, 2, 7, 1, 4, 6, 0], 2), *ROOTS["aniso"]))]


def _raw(H, block, pts, n, flags, out, grad):
    buf = bytes(block)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return H.lib().hpsdf_query_true_gradient_block(buf, len(buf), vp(pts), n, flags, vp(out), vp(grad))


# ------------------------------------------------------------------------------------------------------------ 1
def test_reference_agrees_with_mpmath():
    """sum_i c_i N_a N_b N_c P_a'(x) P_b(y) P_c(z) with mpmath.legendre and mpmath.diff at 40 digits, two dozen points per degree
    0..12: the long-double reference (which runs the recurrence with the reference's float64 constants, each within u/2 of
    (2j-1)/j and (j-1)/j -- a perturbation of the kind the bound's recurrence model allots to every step) lies within its own bound."""
    rng = np.random.default_rng(21)
    worst = 0.0
    for p in range(13):
        blk = synthetic_block(rng, [p] * 8, 1, *ROOTS["cube"])
        B = R.Block(blk)
        pts = R.points_in_leaves(B, rng, 24)
        ref = G.gradient_reference(B, pts)
        q = B.to_unit(pts)
        inv = (np.float32(1.0) / (B.root_max - B.root_min)).astype(np.float64)
        nc = int(R.COUNT[p])
        with mpmath.workdps(40):
            for i in range(len(pts)):
                n = ref["leaf"][i]
                dep = int(B.depth[n])
                cen = ((B.bmin[n] + B.bmax[n]) / np.float32(2.0)).astype(np.float64)
                x = (q[i] - cen) * float(2 << dep)
                P = [[mpmath.legendre(j, mpmath.mpf(float(x[k]))) for j in range(p + 1)] for k in range(3)]
                dP = [[mpmath.diff(lambda t, j=j: mpmath.legendre(j, t), mpmath.mpf(float(x[k]))) for j in range(p + 1)] for k in range(3)]
                co = B.coeffs[B.start[n]:B.start[n] + nc]
                for k in range(3):
                    tot = mpmath.mpf(0)
                    for r in range(nc):
                        idx = R.BIDX[r]
                        term = mpmath.mpf(float(co[r]))
                        for ax in range(3):
                            term *= mpmath.mpf(float(R.NL[idx[ax], dep])) * (dP[ax][idx[ax]] if ax == k else P[ax][idx[ax]])
                        tot += term
                    tot *= mpmath.mpf(float(2 << dep)) * mpmath.mpf(float(inv[k]))
                    gk = ref["g"][i, k]
                    err = float(abs(mpmath.mpf(float(gk)) + mpmath.mpf(float(gk - R.LD(float(gk)))) - tot))
                    assert err <= ref["g_bound"][i, k], (p, i, k, err / ref["g_bound"][i, k])
                    worst = max(worst, err)
    assert worst > 0


# ------------------------------------------------------------------------------------------------------------ 2, 3
def test_block_entry_within_the_bound(H):
    rng = np.random.default_rng(23)
    for name, blk in gradient_blocks(rng):
        pts = R.points_in_leaves(blk, rng, 512)
        ref = G.gradient_reference(blk, pts, left=bool(H.reduction_order()))
        for unit in (False, True):
            v, g = H.query_gradient_block(blk, pts, unit=unit)
            ex = G.excess(g, ref, unit)
            print(name, "unit" if unit else "world", "excess %.3g" % ex)
            assert ex <= 1, (name, unit, ex)


def test_value_output_is_query_bit_for_bit(H, O):
    rng = np.random.default_rng(29)
    for name, blk in gradient_blocks(rng):
        B = R.Block(blk)
        pts = np.concatenate([R.points_in_leaves(B, rng, 512), B.from_unit(edge_points(rng))])
        want = O.Tree.from_block(blk).query(pts)
        got, g = H.query_gradient_block(blk, pts)
        assert np.array_equal(_bits(got), _bits(want)), name
        outside = want == DBL_MAX
        assert outside.any() and np.isnan(g[outside]).all() and np.isfinite(g[~outside]).all(), name


# ------------------------------------------------------------------------------------------------------------ 4
def test_bound_rejects_the_shortcut(H, O):
    """QueryWithGradient's vector -- the reference's per-axis shortcut -- is not the gradient: normalised (the oracle's output) it
    leaves the unit bound, unnormalised and pushed through the same world scaling it leaves the world bound, on every block."""
    rng = np.random.default_rng(31)
    for name, blk in gradient_blocks(rng):
        B = R.Block(blk)
        lv = B.leaves()
        if (B.degree[lv] == 0).all():
            continue
        pts = R.points_in_leaves(B, rng, 200)
        ref_w = G.gradient_reference(B, pts)
        _, gs = O.Tree.from_block(blk).query_with_gradient(pts)
        raw = G.shortcut_unnormalised(B, pts)
        nrm = np.sqrt((raw ** 2).sum(1))
        ok = nrm > 0
        assert np.abs((raw[ok] / nrm[ok, None]).astype(np.float64) - gs[ok]).max() < 1e-6, name   # the helper restates the shortcut
        inv = (np.float32(1.0) / (B.root_max - B.root_min)).astype(np.float64)
        world = raw.astype(np.float64) * (2 << B.depth[ref_w["leaf"]]).astype(np.float64)[:, None] * inv
        assert G.excess(gs, ref_w, unit=True) > 1 and G.excess(world, ref_w) > 1, name


def test_bound_rejects_a_scaled_derivative_constant():
    """D_2 = D_0 + 3 (1 + 2^-40) L_1: at leaves of degree >= 2 the mutant leaves the bound in every block."""
    rng = np.random.default_rng(37)
    for rmin, rmax in (ROOTS["unit"], ROOTS["cube"], ROOTS["aniso"]):
        for degs in ([2] * 8, [3] * 8, [5] * 8, [12] * 8):
            blk = synthetic_block(rng, degs, 1, rmin, rmax)
            pts = R.points_in_leaves(blk, rng, 100)
            true = G.gradient_reference(blk, pts)
            mut = G.gradient_reference(blk, pts, dscale={2: 1.0 + 2.0 ** -40})
            assert G.excess(mut["g"].astype(np.float64), true) > 1, (rmin, degs[0])
            d = np.abs(mut["g"] - true["g"]).astype(np.float64)
            assert (d / true["g_bound"]).max() > 1


def test_bound_rejects_the_neighbouring_leaf(H):
    """On a cell face Query answers from the upper cell; the gradient taken from the leaf across the face is another polynomial's."""
    rng = np.random.default_rng(41)
    for rmin, rmax in (ROOTS["unit"], ROOTS["aniso"]):        # (roots whose map is exact on the planes: the points stay ON the faces)
        blk = synthetic_block(rng, [2, 3, 4, 5, 1, 2, 3, 6], 2, rmin, rmax)
        B = R.Block(blk)
        q = rng.uniform(-0.49, 0.49, (96, 3))
        for axis in range(3):
            q[32 * axis:32 * axis + 32, axis] = rng.choice([0.0, -0.25], 32)
        pts = B.from_unit(q)
        face = np.zeros(len(q), bool)
        qq = B.to_unit(pts)
        for axis in range(3):
            face[32 * axis:32 * axis + 32] = np.isin(qq[32 * axis:32 * axis + 32, axis], [0.0, -0.25])
        assert face.all()
        pts, qq = pts[face], qq[face]
        axis_of = np.repeat(np.arange(3), 32)[face]
        true = G.gradient_reference(B, pts)
        other = true["leaf"].copy()
        for axis in range(3):
            m = axis_of == axis
            other[m] = G.lower_neighbour_leaves(B, pts[m], axis)
        moved = other != true["leaf"]
        assert moved.sum() >= 24
        mut = G.gradient_reference(B, pts, leaf=other)
        d = np.abs(mut["g"] - true["g"]).astype(np.float64)
        assert ((d / true["g_bound"]).max(1)[moved] > 1).all()
        _, g = H.query_gradient_block(blk, pts)
        assert G.excess(g, true) <= 1                 # the product answers from the leaf Query answers from


# ------------------------------------------------------------------------------------------------------------ 5, 6
def test_outside_and_nan_rows(H):
    rng = np.random.default_rng(43)
    blk = synthetic_block(rng, list(range(8)), 1)
    pts = rng.uniform(-0.4, 0.4, (12, 3))
    pts[0, 0] = 0.6
    pts[1, 1] = -7.0
    pts[2, 2] = np.nan
    pts[3] = np.nan
    pts[4, 0] = np.inf
    for unit in (False, True):
        v, g = H.query_gradient_block(blk, pts, unit=unit)
        assert (v[:5] == DBL_MAX).all() and np.isnan(g[:5]).all()
        assert (v[5:] != DBL_MAX).all() and np.isfinite(g[5:]).all()


def test_argument_checks(H):
    rng = np.random.default_rng(47)
    blk = synthetic_block(rng, list(range(8)), 1)
    pts = rng.uniform(-0.4, 0.4, (4, 3))
    out, grad = np.full(4, 7.0), np.full((4, 3), 7.0)
    assert _raw(H, blk, pts, 0, 0, out, grad) == H.OK and (grad == 7.0).all()
    assert _raw(H, blk, None, 0, 1, None, None) == H.OK
    assert _raw(H, blk, pts, 4, 2, out, grad) == 1 and b"flag" in H.lib().hpsdf_last_error()          # HPSDF_ERR_INVALID_ARGUMENT
    assert _raw(H, blk, pts, 4, 0x80000001, out, grad) == 1
    assert _raw(H, blk, pts, 4, 0, out, None) == 1 and H.lib().hpsdf_last_error()
    assert (grad == 7.0).all() and (out == 7.0).all()
    for cut in (blk[:-1], blk[:100], blk[:8], b""):
        assert _raw(H, cut, pts, 4, 0, out, grad) == 4 and H.lib().hpsdf_last_error()                  # HPSDF_ERR_BAD_BLOCK
    with pytest.raises(H.HpsdfError):
        H.query_gradient_block(blk[:-8], pts)
    # out = NULL: gradients only, the same rows
    g2 = np.empty((4, 3))
    assert _raw(H, blk, pts, 4, 1, None, g2) == H.OK
    assert np.array_equal(_bits(g2), _bits(H.query_gradient_block(blk, pts, unit=True)[1]))


# ------------------------------------------------------------------------------------------------------------ 7
def test_unit_flag_is_the_stated_normalisation(H):
    rng = np.random.default_rng(53)
    before = H.reduction_order()
    try:
        differ = 0
        for name, blk in gradient_blocks(rng):
            pts = R.points_in_leaves(blk, rng, 512)
            _, g = H.query_gradient_block(blk, pts)
            got = {}
            for left in (0, 1):
                H.set_reduction_order(left)
                _, got[left] = H.query_gradient_block(blk, pts, unit=True)
                a, b, c = g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2]
                z = (a + b) + c if left else a + (b + c)
                with np.errstate(invalid="ignore", divide="ignore"):
                    want = np.where((z > 0)[:, None], g / np.sqrt(z)[:, None], g)
                assert np.array_equal(_bits(got[left]), _bits(want)), (name, left)
                nz = z > 0
                ln = np.sqrt((got[left][nz].astype(R.LD) ** 2).sum(1))
                assert (np.abs(ln - 1).astype(np.float64) <= 4 * R.U).all(), (name, left)
                assert (got[left][~nz] == 0).all()
            differ += int((_bits(got[0]) != _bits(got[1])).any(1).sum())
        assert differ > 0          # the two orders are told apart somewhere
    finally:
        H.set_reduction_order(before)
    assert H.reduction_order() == before


# ------------------------------------------------------------------------------------------------------------ 8
def test_sphere_gradient_is_radial(H, O):
    """The oracle's sphere tree at 1e-8 (centre (0.25, 0, 0), radius 0.5), points ON the true sphere with |coordinate| < 0.49: the
    unit gradient is the outward radial direction, cos >= 0.9999 at every point (0.81 degrees).  The long-double reference alone
    gives 1 - cos <= 4.9e-8 there, so this is an orientation-and-scale check with a margin of 2000, not an accuracy claim; the
    reference's shortcut (QueryWithGradient) is off by 0.9 degrees in the median and fails it."""
    blk = O.Tree.create(O.default_config(1e-8), O.sphere_field(), 1024).to_block()
    rng = np.random.default_rng(59)
    d = rng.standard_normal((4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.array([0.25, 0.0, 0.0]) + 0.5 * d
    keep = (np.abs(pts) < 0.49).all(1)
    pts, d = pts[keep][:400], d[keep][:400]
    assert len(pts) == 400
    v, g = H.query_gradient_block(blk, pts, unit=True)
    cos = (g * d).sum(1)
    print("min cos %.12f, max |value| %.3g" % (cos.min(), np.abs(v).max()))
    assert (cos >= 0.9999).all(), cos.min()
    _, gw = H.query_gradient_block(blk, pts)
    assert np.abs(np.linalg.norm(gw, axis=1) - 1).max() < 1e-2          # a distance field: |grad| = 1 (scale: root size 1)
    _, gs = O.Tree.from_block(blk).query_with_gradient(pts)
    assert not ((gs * d).sum(1) >= 0.9999).all()                         # the shortcut does not pass


# ------------------------------------------------------------------------------------------------------------ 9
def test_save_obj_with_normals_round_trips(H, tmp_path):
    rng = np.random.default_rng(61)
    verts = rng.uniform(-1, 1, (7, 3))
    tris = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.uint64)
    nrm = rng.standard_normal((7, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    plain, withn = str(tmp_path / "plain.obj"), str(tmp_path / "normals.obj")
    H.save_obj(plain, verts, tris)
    v32 = verts.astype(np.float32)
    want = "".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in r) for r in v32) + "".join("f %d %d %d\n" % tuple(int(x) + 1 for x in r) for r in tris)
    assert open(plain, "rb").read() == want.encode()
    H.save_obj(withn, verts, tris, normals=nrm)
    text = open(withn).read().splitlines()
    assert [l.split()[0] for l in text] == ["v"] * 7 + ["vn"] * 7 + ["f"] * 4
    assert text[7] == "vn %.9g %.9g %.9g" % tuple(nrm[0]) and text[14] == "f 1//1 2//2 3//3"
    for path in (plain, withn):
        lv, lt = H.load_obj(path)
        assert np.array_equal(lv, v32) and np.array_equal(lt, tris)
    with pytest.raises(ValueError):
        H.save_obj(withn, verts, tris, normals=nrm[:3])
