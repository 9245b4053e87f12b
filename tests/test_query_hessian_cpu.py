"""QueryHessian without a device: hpsdf_query_hessian_block (the statements of the kernels on the calling thread) against the
long-double reference of tests/hiprec_hessian.py and its derived bound, the reference's second derivative against numpy's legder,
mutants the bound rejects, values and gradients against Query and QueryGradient bit for bit, the curvature against a float64
restatement bit for bit, the argument checks, and the curvature of a built sphere."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from numpy.polynomial import legendre as npleg

import hiprec as R
import hiprec_gradient as G
import hiprec_hessian as HS
from conftest import ROOT
from helpers import block_reader_table, edge_points, synthetic_block
from test_hiprec_cpu import ROOTS, _with_root, query_blocks

DBL_MAX = np.finfo(np.float64).max
NAN_BITS = np.uint64(0x7FF8000000000000)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def hessian_blocks(rng):
    """query_blocks (every degree 0..12, depths to 10, the unit root and [-0.25, 5]^3), a block on an anisotropic root, and the
    synthetic trees of tests/test_gpu_query_gradient.py whose largest degree is 2 (all leaves in the top table; and not), 3, 5 and 12."""
    out = query_blocks(rng)
    out.append(("aniso", _with_root(synthetic_block(rng, [3, 5, 2, 7, 1, 4, 6, 0], 2), *ROOTS["aniso"])))
    out.append(("max2-top", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 1)))
    out.append(("max2", synthetic_block(rng, [2, 1, 0, 2, 2, 1, 2, 0], 2, *ROOTS["cube"])))
    out.append(("max3", synthetic_block(rng, [3, 2, 1, 0, 3, 3, 2, 1], 2)))
    out.append(("max5", synthetic_block(rng, [5, 4, 3, 2, 1, 0, 5, 4], 2, *ROOTS["cube"])))
    out.append(("max12", synthetic_block(rng, [12, 7, 3, 2, 9, 0, 5, 6], 2)))
    return out


def _raw(H, block, pts, n, flags, out, grad, hess, curv):
    buf = bytes(block)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return H.lib().hpsdf_query_hessian_block(buf, len(buf), vp(pts), n, flags, vp(out), vp(grad), vp(hess), vp(curv))


def curvature_f64(g, H, left):
    """The stated statements in numpy float64 (+, -, *, / and sqrt are correctly rounded there as in the library)."""
    return HS.curvature_ld(np.asarray(g, np.float64), np.asarray(H, np.float64), bool(left))


# ------------------------------------------------------------------------------------------------------------ the reference itself
def test_reference_second_derivative_is_legder():
    """E_j of the reference (the stated recurrence, long double, on D_j and L_j run with the reference's float64 constants) against
    d^2/dx^2 P_j from numpy.polynomial.legendre.legder(.., 2), evaluated in long double, for j <= 12 at 65 points of [-1, 1]: they
    agree within the bound's own model u eE_j (which allots j^2 u to every L_j -- the float64 constants are each within u/2 of
    (2j-1)/j and (j-1)/j) plus the long-double evaluation of the series (2^-64 per operation, a few hundred operations on terms no
    larger than the sum of |E_k|: 2^-54 (1 + |E_j|) is generous)."""
    xs = np.concatenate([np.linspace(-1.0, 1.0, 33), np.random.default_rng(3).uniform(-1, 1, 32)])
    worst = 0.0
    for x in xs:
        L = R.legendre_ld(np.array([x]), 12)[:, 0]
        D = G.derivative_ld(L, 12)
        E = HS.second_derivative_ld(D, 12)
        La, Da, Ea = (np.abs(v).astype(np.float64) for v in (L, D, E))
        eE = HS.second_derivative_error_units(Da, Ea, G.derivative_error_units(La, Da, 12), 12)
        for j in range(13):
            c = np.zeros(j + 1, R.LD)
            c[j] = 1
            d2 = npleg.legder(c, 2)
            want = npleg.legval(R.LD(x), d2) if len(d2) else R.LD(0)
            err = abs(float(E[j] - want))
            assert err <= R.U * eE[j] * R.SLACK + 2.0 ** -54 * (1 + Ea[j]), (j, x, err)
            worst = max(worst, err / max(1.0, Ea[j]))
    assert npleg.legder(np.array([0, 0, 1], R.LD), 2).dtype == R.LD
    assert worst < 1e-12      # the agreement is to long-double-scale accuracy, not merely to the bound


# ------------------------------------------------------------------------------------------------------------ the bound
def test_block_entry_within_the_bound(H):
    rng = np.random.default_rng(211)
    degrees = set()
    for name, blk in hessian_blocks(rng):
        B = R.Block(blk)
        degrees.add(int(B.degree[B.leaves()].max()))
        pts = R.points_in_leaves(B, rng, 256)
        ref = HS.hessian_reference(B, pts, left=bool(H.reduction_order()))
        v, g, hs = H.query_hessian_block(blk, pts)
        ex = HS.excess(hs, ref)
        print(name, "excess %.3g" % ex)
        assert ex <= 1, (name, ex)
    assert {2, 3, 5, 12} <= degrees


def test_bound_rejects_a_scaled_second_derivative_constant():
    """E_j = E_{j-2} + (2j-1) (1 + 2^-40) D_{j-1} for one j: the mutant leaves the bound in every block of leaves of degree p >= 2, for
    j = p (the top term, which the bound's own allowance is relative to), and for j = 2 up to p = 5.  (At p = 12 the j = 2 mutant
    moves the entries by 2^-40 of their E_2, E_4, .. parts only, which the rounding allowance of the terms of degree 11 and 12
    legitimately exceeds; it is not asserted there.)"""
    rng = np.random.default_rng(223)
    for rmin, rmax in (ROOTS["unit"], ROOTS["cube"], ROOTS["aniso"]):
        for p in (2, 3, 5, 12):
            blk = synthetic_block(rng, [p] * 8, 1, rmin, rmax)
            pts = R.points_in_leaves(blk, rng, 100)
            true = HS.hessian_reference(blk, pts)
            for j in sorted({p, 2 if p <= 5 else p}):
                mut = HS.hessian_reference(blk, pts, escale={j: 1.0 + 2.0 ** -40})
                d = np.abs(mut["H"] - true["H"]).astype(np.float64)
                assert (d / true["H_bound"]).max() > 1 and HS.excess(mut["H"].astype(np.float64), true) > 1, (rmin, p, j)


def test_bound_rejects_swapped_xz_and_yz(H):
    rng = np.random.default_rng(227)
    for name, blk in hessian_blocks(rng):
        pts = R.points_in_leaves(blk, rng, 100)
        true = HS.hessian_reference(blk, pts)
        _, _, hs = H.query_hessian_block(blk, pts)
        assert HS.excess(hs, true) <= 1 and HS.excess(hs[:, [0, 1, 2, 3, 5, 4]], true) > 1, name


def test_bound_rejects_the_neighbouring_leaf(H):
    """On a cell face Query answers from the upper cell; the Hessian taken from the leaf across the face is another polynomial's
    (every leaf here has degree >= 2: two leaves of degree <= 1 share the Hessian zero)."""
    rng = np.random.default_rng(229)
    for rmin, rmax in (ROOTS["unit"], ROOTS["aniso"]):        # (roots whose map is exact on the planes: the points stay ON the faces)
        blk = synthetic_block(rng, [2, 3, 4, 5, 2, 2, 3, 6], 2, rmin, rmax)
        B = R.Block(blk)
        q = rng.uniform(-0.49, 0.49, (96, 3))
        for axis in range(3):
            q[32 * axis:32 * axis + 32, axis] = rng.choice([0.0, -0.25], 32)
        pts = B.from_unit(q)
        qq = B.to_unit(pts)
        axis_of = np.repeat(np.arange(3), 32)
        assert all(np.isin(qq[axis_of == a, a], [0.0, -0.25]).all() for a in range(3))
        true = HS.hessian_reference(B, pts)
        other = true["leaf"].copy()
        for axis in range(3):
            m = axis_of == axis
            other[m] = G.lower_neighbour_leaves(B, pts[m], axis)
        moved = other != true["leaf"]
        assert moved.sum() >= 24
        mut = HS.hessian_reference(B, pts, leaf=other)
        d = np.abs(mut["H"] - true["H"]).astype(np.float64)
        assert ((d / true["H_bound"]).max(1)[moved] > 1).all()
        _, _, hs = H.query_hessian_block(blk, pts)
        assert HS.excess(hs, true) <= 1                 # the product answers from the leaf Query answers from


def test_bound_rejects_one_axis_scaling_applied_twice():
    """H_ab scaled by rootInvSizes[a] twice in place of [a] and [b]: on the anisotropic root every mixed entry leaves the bound."""
    rng = np.random.default_rng(233)
    blk = synthetic_block(rng, [3, 5, 2, 7, 2, 4, 6, 2], 2, *ROOTS["aniso"])
    pts = R.points_in_leaves(blk, rng, 100)
    true = HS.hessian_reference(blk, pts)
    mut = HS.hessian_reference(blk, pts, inv_twice=True)
    d = np.abs(mut["H"] - true["H"]).astype(np.float64)
    assert ((d / true["H_bound"])[:, 3:].max(1) > 1).all() and HS.excess(mut["H"].astype(np.float64), true) > 1
    assert (d[:, :3] == 0).all()


# ------------------------------------------------------------------------------------------------------------ the other outputs
def test_values_and_gradients_are_query_and_query_gradient_bit_for_bit(H, O):
    rng = np.random.default_rng(239)
    before = H.reduction_order()
    try:
        for name, blk in hessian_blocks(rng):
            B = R.Block(blk)
            pts = np.concatenate([R.points_in_leaves(B, rng, 512), B.from_unit(edge_points(rng))])
            want = O.Tree.from_block(blk).query(pts)
            outside = want == DBL_MAX
            assert outside.any()
            for left in (0, 1):
                H.set_reduction_order(left)
                h0 = None
                for unit in (False, True):
                    gv, gg = H.query_gradient_block(blk, pts, unit=unit)
                    v, g, hs, cv = H.query_hessian_block(blk, pts, unit=unit, curvature=True)
                    assert np.array_equal(_bits(v), _bits(want)) and np.array_equal(_bits(gv), _bits(want)), (name, left, unit)
                    assert np.array_equal(_bits(g), _bits(gg)), (name, left, unit)
                    assert np.isnan(hs[outside]).all() and np.isnan(cv[outside]).all() and np.isfinite(hs[~outside]).all()
                    if h0 is None:
                        h0 = (hs, cv)
                    else:           # the unit flag touches the gradient row alone
                        assert np.array_equal(_bits(hs), _bits(h0[0])) and np.array_equal(_bits(cv), _bits(h0[1])), (name, left)
    finally:
        H.set_reduction_order(before)


def test_curvature_is_the_stated_statements_bit_for_bit(H):
    rng = np.random.default_rng(241)
    before = H.reduction_order()
    try:
        differ = 0
        for name, blk in hessian_blocks(rng):
            pts = R.points_in_leaves(blk, rng, 512)
            got = {}
            for left in (0, 1):
                H.set_reduction_order(left)
                v, g, hs, cv = H.query_hessian_block(blk, pts, curvature=True)
                want = curvature_f64(g, hs, left)
                assert np.array_equal(_bits(cv), _bits(want)), (name, left)
                z = HS._sum3(g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2], left)
                assert (_bits(cv[~(z > 0)]) == NAN_BITS).all() and np.isfinite(cv[z > 0]).all(), (name, left)
                got[left] = cv
            differ += int((_bits(got[0]) != _bits(got[1])).any(1).sum())
        assert differ > 0          # the two orders are told apart somewhere
    finally:
        H.set_reduction_order(before)


def test_zero_gradient_rows_are_nan(H):
    rng = np.random.default_rng(251)
    blk = synthetic_block(rng, [0] * 8, 1)
    pts = rng.uniform(-0.49, 0.49, (64, 3))
    v, g, hs, cv = H.query_hessian_block(blk, pts, unit=True, curvature=True)
    assert (v != DBL_MAX).all() and (g == 0).all() and (hs == 0).all() and (_bits(cv) == NAN_BITS).all()
    blk = synthetic_block(rng, [1] * 8, 1)                  # degree 1: a zero Hessian, hence a flat level set
    v, g, hs, cv = H.query_hessian_block(blk, pts, curvature=True)
    assert (hs == 0).all() and (np.abs(g).max(1) > 0).all() and (cv == 0).all()


def test_outside_nan_and_inf_rows(H):
    rng = np.random.default_rng(257)
    blk = synthetic_block(rng, [2, 3, 4, 5, 6, 7, 2, 3], 1)
    pts = rng.uniform(-0.4, 0.4, (12, 3))
    pts[0, 0] = 0.6
    pts[1, 1] = -7.0
    pts[2, 2] = np.nan
    pts[3] = np.nan
    pts[4, 0] = np.inf
    pts[5] = -np.inf
    for unit in (False, True):
        v, g, hs, cv = H.query_hessian_block(blk, pts, unit=unit, curvature=True)
        assert (v[:6] == DBL_MAX).all()
        for a in (g, hs, cv):
            assert (_bits(a[:6]) == NAN_BITS).all() and np.isfinite(a[6:]).all()
        assert (v[6:] != DBL_MAX).all()


# ------------------------------------------------------------------------------------------------------------ arguments
def test_null_outputs_and_argument_checks(H):
    rng = np.random.default_rng(263)
    blk = synthetic_block(rng, [2, 3, 4, 5, 6, 7, 2, 3], 1)
    pts = rng.uniform(-0.4, 0.4, (4, 3))
    full = H.query_hessian_block(blk, pts, unit=True, curvature=True)
    fresh = lambda: [np.full(4, 7.0), np.full((4, 3), 7.0), np.full((4, 6), 7.0), np.full((4, 2), 7.0)]
    # every combination of NULL outputs that keeps hess or curv: the arrays asked for are the full call's, nothing else is written
    for mask in range(16):
        bufs = fresh()
        args = [b if mask >> k & 1 else None for k, b in enumerate(bufs)]
        rc = _raw(H, blk, pts, 4, 1, *args)
        if args[2] is None and args[3] is None:
            assert rc == H.ERR_INVALID_ARGUMENT and H.lib().hpsdf_last_error() and all((b == 7.0).all() for b in bufs), mask
            continue
        assert rc == H.OK, mask
        for k in range(4):
            if args[k] is None:
                assert (bufs[k] == 7.0).all(), (mask, k)
            else:
                assert np.array_equal(_bits(bufs[k]), _bits(full[k])), (mask, k)
    bufs = fresh()
    untouched = lambda: all((b == 7.0).all() for b in bufs)
    assert _raw(H, blk, pts, 0, 0, *bufs) == H.OK and untouched()
    assert _raw(H, blk, None, 0, 1, None, None, bufs[2], None) == H.OK
    assert _raw(H, blk, pts, 4, 2, *bufs) == H.ERR_INVALID_ARGUMENT and b"flag" in H.lib().hpsdf_last_error() and untouched()
    assert _raw(H, blk, pts, 4, 0x80000001, *bufs) == H.ERR_INVALID_ARGUMENT and untouched()
    assert _raw(H, blk, None, 4, 0, *bufs) == H.ERR_INVALID_ARGUMENT and H.lib().hpsdf_last_error() and untouched()
    # blocks are accepted and refused exactly as hpsdf_query_true_gradient_block accepts and refuses them
    status = {"ok": H.OK, "bad_block": H.ERR_BAD_BLOCK, "unsupported": H.ERR_UNSUPPORTED}
    for name, b, st in block_reader_table():
        grad = np.full((4, 3), 7.0)
        want = H.lib().hpsdf_query_true_gradient_block(bytes(b), len(b), pts.ctypes.data_as(C.c_void_p), 4, 0, None, grad.ctypes.data_as(C.c_void_p))
        bufs = fresh()
        assert _raw(H, b, pts, 4, 0, *bufs) == want == status[st], name
        assert (st == "ok") != untouched(), name
    with pytest.raises(H.HpsdfError) as ei:
        H.query_hessian_block(blk[:-8], pts)
    assert ei.value.status == H.ERR_BAD_BLOCK


def test_new_symbols_are_declared_bound_and_exported(H):
    hdr = open(os.path.join(ROOT, "include", "hpsdf.h")).read()
    declared = set(re.findall(r"HPSDF_API\s+[\w\s\*]+?\b(hpsdf_\w+)\s*\(", hdr))
    new = {"hpsdf_query_hessian_device", "hpsdf_query_hessian_host", "hpsdf_query_hessian_block"}
    assert new <= declared and new <= set(H._SIGNATURES)
    for name in new:
        assert hasattr(H.lib(), name)
    assert H.ABI_VERSION == 4 and H.lib().hpsdf_abi_version() == 4
    assert int(re.search(r"#define HPSDF_ABI_VERSION (\d+)", hdr).group(1)) == 4


# ------------------------------------------------------------------------------------------------------------ a built sphere
def test_sphere_curvature(H, O):
    """The oracle's sphere tree at 1e-8 (centre (0.25, 0, 0), radius 0.5, as tests/test_project_cpu.py builds it), the converged rows of
    project_block from points uniform in [-0.49, 0.49]^3 -- points ON the fitted level set: the product's mean curvature is 2 = 1/r and
    its Gaussian curvature 4 = 1/r^2 (field positive outside) within twice the deviation the long-double reference itself shows on
    those points.  That deviation is the fit's error -- the tree approximates the sphere piecewise -- not rounding; it has to come out
    below 0.25 (mean) and 0.5 (gauss), so that the tolerances stay below 0.5 and 1 and a wrong sign or a factor of 2 fails.
    Measured when this was written: the 300 points lie in leaves of degree 3; the reference deviates from (2, 4) by at most 0.0229
    (mean) and 0.0913 (gauss), so the tolerances are 0.046 and 0.18; the product shows the same 0.0229 and 0.0913."""
    blk = O.Tree.create(O.default_config(1e-8), O.sphere_field(), 1024).to_block()
    rng = np.random.default_rng(269)
    pts = rng.uniform(-0.49, 0.49, (1200, 3))
    x, val, grad, iters, status = H.project_block(blk, pts, 0.0, 1e-9, 16)
    on = x[status == H.PROJECT_CONVERGED][:300]
    assert len(on) == 300
    B = R.Block(blk)
    ref = HS.hessian_reference(B, on, left=bool(H.reduction_order()))
    dev_mean = float(np.abs(ref["curv"][:, 0] - 2).max())
    dev_gauss = float(np.abs(ref["curv"][:, 1] - 4).max())
    v, g, hs, cv = H.query_hessian_block(blk, on, curvature=True)
    err_mean, err_gauss = float(np.abs(cv[:, 0] - 2).max()), float(np.abs(cv[:, 1] - 4).max())
    print("leaf degrees %s; reference deviation: mean %.3g, gauss %.3g; product: mean %.3g, gauss %.3g; Hessian excess %.3g"
          % (sorted(set(B.degree[ref["leaf"]].tolist())), dev_mean, dev_gauss, err_mean, err_gauss, HS.excess(hs, ref)))
    assert 2 * dev_mean < 0.5 and 2 * dev_gauss < 1.0, (dev_mean, dev_gauss)
    assert err_mean <= 2 * dev_mean and err_gauss <= 2 * dev_gauss
    assert HS.excess(hs, ref) <= 1
