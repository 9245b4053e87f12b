"""The two surface extractions at the smallest lattices: less than one 8^3 block, exactly one block, one cube past a block -- where the
helpers both calls share (csrc/surface_common.hpp) meet the dense call's edge words and the sparse call's block-local indices.  The
dense mesh against the numpy restatement (tests/surface_reference.py) on the returned lattice values, the sparse mesh against the
dense one, both bit for bit, and the device's block classes against the host's."""
import numpy as np
import pytest

import surface_reference as S

pytestmark = pytest.mark.gpu

SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.3
SPHERE_TARGET = 1e-6


def box(lo_off, hi_off):
    return tuple(c + lo_off for c in SPHERE_C), tuple(c + hi_off for c in SPHERE_C)


# A = [c, c + 0.4]: the lower corner is the sphere's centre; every other lattice point on the three axes through it is at least 0.4 / n
# away along an axis and the far corner is outside (0.4 > r), so an edge crosses even at n = 1.
# B = [c - 0.2, c + 0.2]: the face centres are 0.2 from c (inside), the corners 0.346 (outside) -- the surface crosses all six faces, so
# the last block of every axis owns crossing edges of the boundary layer.
BOX_A, BOX_B = box(0.0, 0.4), box(-0.2, 0.2)
CASES = [
    (BOX_A, (1, 1, 1)),
    (BOX_A, (1, 17, 8)),
    (BOX_A, (16, 9, 1)),
    (BOX_B, (8, 8, 8)),
    (BOX_B, (9, 8, 7)),
    (BOX_B, (7, 9, 16)),
]


@pytest.fixture(scope="module")
def sphere(H, ctx):
    block, _ = H.create_block(ctx, H.make_config(SPHERE_TARGET), H.Field.sphere(SPHERE_C, SPHERE_R), 0)
    t = H.DeviceTree(ctx, block)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("bx,n", CASES)
def test_small_lattices_dense_is_the_restatement_and_sparse_is_dense(H, sphere, bx, n):
    lo, hi = bx
    dv, dt, vals = sphere.extract_surface(lo, hi, n, 0.0, values=True)
    rv, rt = S.extract(vals, lo, hi, n, 0.0, H.surface_case_table())
    print(n, "verts", len(dv), "tris", len(dt), "restatement", len(rv), len(rt))
    assert len(dt) > 0
    assert dv.shape == rv.shape and dt.shape == rt.shape
    assert np.array_equal(bits(dv), bits(rv)), "dense vertex bits differ from the restatement"
    assert np.array_equal(dt, rt), "dense triangles differ from the restatement"
    sv, st = sphere.extract_surface_sparse(lo, hi, n, 0.0)
    assert sv.shape == dv.shape and st.shape == dt.shape
    assert np.array_equal(bits(sv), bits(dv)), "sparse vertex bits differ from the dense call's"
    assert np.array_equal(st, dt), "sparse triangles differ from the dense call's"
    dev = sphere.classify_surface_blocks(lo, hi, n, 0.0)
    host = H.surface_classify_host(sphere.block, lo, hi, n, 0.0)
    assert dev.shape == host.shape == (H.surface_block_count(n),)
    assert np.array_equal(dev, host)
    if n == (1, 1, 1):  # one corner inside, seven outside: the corner is cut off by one triangle
        assert int((vals < 0.0).sum()) == 1 and vals[0, 0, 0] < 0.0
        assert len(dt) == 1 and len(dv) == 3
