"""The *_host entries of QueryGradient, QueryHessian, ProjectToSurface and CastRays with every subset of their optional outputs, at one
size for each of the three ways a host call moves its arrays (csrc/host_call.hpp, hostCall): each array passed equals the device-free
_block entry's bit for bit, whichever arrays go with it.  An entry that handed the kernel one output's device array for another's would
pass every other test here: those either pass all the outputs or go through the _device entries."""
import ctypes as C
import itertools

import numpy as np
import pytest

import hiprec as R
from test_cast_rays_cpu import cast_levels, cast_rays
from test_gpu_query_gradient import _point_set, _trees

# Restated from csrc/host_call.hpp: a call's arrays are laid out one after the other, each rounded up to 256 bytes; up to kZeroCopyBytes in
# all the kernel works on the pinned buffer itself, up to kPinnedPathBytes the arrays are staged through it, beyond that they are copied
# between the caller's memory and the device directly.
ZERO_COPY_BYTES, PINNED_PATH_BYTES, ALIGN = 4096, 1 << 20, 256
ROWS_FEW, ROWS_MID = 33, 4096 + 37  # (both past the 32 rows that an entry answers on the calling thread)


def _path(row_bytes, n):
    total = sum((n * b + ALIGN - 1) // ALIGN * ALIGN for b in row_bytes)
    return "zero-copy" if total <= ZERO_COPY_BYTES else "staged" if total <= PINNED_PATH_BYTES else "direct"


def _smallest_direct(row_bytes):
    n = (PINNED_PATH_BYTES - ALIGN * len(row_bytes)) // sum(row_bytes)  # (rounding up adds less than ALIGN an array)
    while _path(row_bytes, n) != "direct":
        n += 1
    assert _path(row_bytes, n - 1) == "staged"
    return n


def _masks(k, keep=lambda m: True):
    return [m for m in itertools.product((False, True), repeat=k) if keep(m)]


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


class _Entry:
    """One _host entry: the bytes a row of its inputs, its required outputs and its optional outputs take, and how it is called."""

    def __init__(self, name, in_bytes, required, optional, masks):
        self.name, self.in_bytes, self.required, self.optional, self.masks = name, in_bytes, required, optional, masks
        self.full = in_bytes + [b for _, b in required + optional]
        self.largest = _smallest_direct(self.full)
        self.sizes = (ROWS_FEW, ROWS_MID, self.largest)

    def row_bytes(self, mask):
        return self.in_bytes + [b for _, b in self.required] + [b for (_, b), on in zip(self.optional, mask) if on]

    def check(self, call, want):
        """call(n, outputs by name) runs the entry; want: every output by name from the _block entry, for the largest size."""
        fewest = min(self.masks, key=sum)
        assert [_path(self.row_bytes(fewest), ROWS_FEW), _path(self.full, ROWS_MID), _path(self.full, self.largest)] == \
            ["zero-copy", "staged", "direct"], self.name
        paths = set()
        for n in self.sizes:
            for mask in self.masks:
                names = [k for k, _ in self.required] + [k for (k, _), on in zip(self.optional, mask) if on]
                got = {k: np.full_like(want[k][:n], 7) for k in names}
                assert call(n, got) == 0, (self.name, n, names)
                for k in names:
                    bad = np.nonzero((_raw(got[k]) != _raw(want[k][:n])).any(1))[0]
                    assert len(bad) == 0, (self.name, n, names, k, bad[:8])
                paths.add(_path(self.row_bytes(mask), n))
        assert paths == {"zero-copy", "staged", "direct"}, self.name


@pytest.fixture(scope="module")
def max5(H, ctx):
    blk = dict(_trees(np.random.default_rng(307)))["max5"]
    tree = H.DeviceTree(ctx, blk)
    assert tree.info()["max_degree"] == 5
    yield blk, tree
    tree.close()


def _points(blk, rng, n):
    pts = np.concatenate([_point_set(blk, rng), R.points_in_leaves(R.Block(blk), rng, n)])[:n]
    return np.ascontiguousarray(pts)


@pytest.mark.gpu
def test_query_gradient_host_with_and_without_out(H, ctx, max5):
    (blk, tree), rng = max5, np.random.default_rng(311)
    e = _Entry("hpsdf_query_true_gradient_host", [24], [("grad", 24)], [("out", 8)], _masks(1))
    pts = _points(blk, rng, e.largest)
    out, grad = H.query_gradient_block(blk, pts)
    e.check(lambda n, o: H.lib().hpsdf_query_true_gradient_host(ctx.handle, tree.handle, _vp(pts), n, 0, _vp(o.get("out")), _vp(o["grad"])),
            {"out": out, "grad": grad})


@pytest.mark.gpu
def test_query_hessian_host_every_subset_of_the_outputs(H, ctx, max5):
    (blk, tree), rng = max5, np.random.default_rng(313)
    optional = [("out", 8), ("grad", 24), ("hess", 48), ("curv", 16)]
    e = _Entry("hpsdf_query_hessian_host", [24], [], optional, _masks(4, lambda m: m[2] or m[3]))
    assert len(e.masks) == 12
    pts = _points(blk, rng, e.largest)
    want = dict(zip(("out", "grad", "hess", "curv"), H.query_hessian_block(blk, pts, curvature=True)))
    e.check(lambda n, o: H.lib().hpsdf_query_hessian_host(ctx.handle, tree.handle, _vp(pts), n, 0, *[_vp(o.get(k)) for k, _ in optional]), want)


@pytest.mark.gpu
def test_project_host_every_subset_of_the_outputs_and_in_place(H, ctx, max5):
    (blk, tree), rng = max5, np.random.default_rng(317)
    optional = [("val", 8), ("grad", 24), ("iters", 1), ("status", 1)]
    e = _Entry("hpsdf_project_host", [24], [("xyz", 24)], optional, _masks(4))
    assert len(e.masks) == 16
    pts = _points(blk, rng, e.largest)
    want = dict(zip(("xyz", "val", "grad", "iters", "status"), H.project_block(blk, pts, 0.0, 1e-9, 16)))
    assert len(np.unique(want["status"])) > 1
    host = lambda src, n, o: H.lib().hpsdf_project_host(ctx.handle, tree.handle, _vp(src), n, 0.0, 1e-9, 16, 0, _vp(o["xyz"]),
                                                        *[_vp(o.get(k)) for k, _ in optional])
    e.check(lambda n, o: host(pts, n, o), want)
    # in place: out_xyz is xyz
    for n, path in ((ROWS_FEW, "zero-copy"), (e.largest, "direct")):
        assert _path(e.full, n) == path
        got = {k: np.full_like(want[k][:n], 7) for k in want}
        got["xyz"] = pts[:n].copy()
        assert host(got["xyz"], n, got) == 0
        for k in want:
            assert np.array_equal(_raw(got[k]), _raw(want[k][:n])), ("in place", n, k)


@pytest.mark.gpu
def test_cast_rays_host_every_subset_of_the_outputs(H, ctx, max5):
    (blk, tree), rng = max5, np.random.default_rng(331)
    optional = [("t", 8), ("xyz", 24), ("val", 8), ("grad", 24), ("evals", 2), ("cells", 2)]
    e = _Entry("hpsdf_cast_rays_host", [24, 24, 8], [("status", 1)], optional, _masks(6))
    assert len(e.masks) == 64
    o, d, tm = (np.ascontiguousarray(a[:e.largest]) for a in cast_rays(blk, rng, e.largest))
    assert len(o) == e.largest
    _, tol = cast_levels(H, blk, rng)
    want = dict(zip(("status", "t", "xyz", "val", "grad", "evals", "cells"), H.cast_rays_block(blk, o, d, tm, 0.0, tol, 32, 4096)))
    assert len(np.unique(want["status"])) > 1
    e.check(lambda n, out: H.lib().hpsdf_cast_rays_host(ctx.handle, tree.handle, _vp(o), _vp(d), _vp(tm), n, 0.0, tol, 32, 4096, 0,
                                                         _vp(out["status"]), *[_vp(out.get(k)) for k, _ in optional]), want)
