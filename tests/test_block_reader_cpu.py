"""One reader for a MemoryBlock (csrc/block.hpp): the entry points that take serialised bytes without a device accept the same blocks
and refuse the others with the same status, a message, and nothing written.  CPU only."""
import ctypes as C

import numpy as np

from helpers import block_reader_table

# The continuity calls never read a node's box: a block whose boxes the query paths refuse is an ordinary block to them (HPSDF_OK,
# what they returned for these two rows before the readers were merged).
CONTINUITY_ON_BOXES = 0
N = 4
LO, HI, CUBES = (-0.5,) * 3, (0.5,) * 3, (16,) * 3  # 2 x 2 x 2 blocks of 8^3 cubes


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _entries(H):
    """name -> (call(block) -> status, after filling the outputs with a sentinel; untouched() -> bool; reads the boxes)"""
    L = H.lib()
    pts = np.random.default_rng(5).uniform(-0.4, 0.4, (N, 3))
    out = {}

    def sentinel(*shapes_dtypes):
        return [np.full(s, 7, d) for s, d in shapes_dtypes]

    def refill(bufs):
        for a in bufs:
            a.fill(7)

    def gradient():
        bufs = sentinel((N, np.float64), ((N, 3), np.float64))
        return (lambda b: refill(bufs) or L.hpsdf_query_true_gradient_block(b, len(b), _vp(pts), N, 0, *[_vp(a) for a in bufs]),
                lambda: all((a == 7).all() for a in bufs))

    def project():
        bufs = sentinel(((N, 3), np.float64), (N, np.float64), ((N, 3), np.float64), (N, np.uint8), (N, np.uint8))
        return (lambda b: refill(bufs) or L.hpsdf_project_block(b, len(b), _vp(pts), N, 0.0, 1e-9, 16, 0, *[_vp(a) for a in bufs]),
                lambda: all((a == 7).all() for a in bufs))

    def classify():
        bufs = sentinel((8, np.uint8))
        lo3, hi3, n3 = (C.c_double * 3)(*LO), (C.c_double * 3)(*HI), (C.c_uint32 * 3)(*CUBES)
        return (lambda b: refill(bufs) or L.hpsdf_surface_classify_host(b, len(b), lo3, hi3, n3, 0.0, 0, 8, _vp(bufs[0])),
                lambda: (bufs[0] == 7).all())

    def post_process():
        state = {}

        def call(b):
            state["in"], state["buf"] = b, C.create_string_buffer(b, len(b))
            return L.hpsdf_continuity_post_process(state["buf"], len(b), 0.0, 0, 1, C.byref(H.ContinuityStats()))
        return call, lambda: state["buf"].raw == state["in"]

    def matrix():
        state = {}

        def call(b):
            ptrs = state["ptrs"] = [C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_double)()]
            rc = L.hpsdf_continuity_matrix(b, len(b), 1, *[C.byref(p) for p in ptrs], C.byref(H.ContinuityStats()))
            if rc == 0:
                for p in ptrs:
                    L._libc.free(C.cast(p, C.c_void_p))
            return rc
        return call, lambda: not any(state["ptrs"])

    for name, make, boxes in (("hpsdf_query_true_gradient_block", gradient, True), ("hpsdf_project_block", project, True),
                              ("hpsdf_surface_classify_host", classify, True), ("hpsdf_continuity_post_process", post_process, False),
                              ("hpsdf_continuity_matrix", matrix, False)):
        out[name] = make() + (boxes,)
    return out


def test_every_reader_gives_the_same_verdict(H):
    L = H.lib()
    table = block_reader_table()
    STATUS = {"ok": H.OK, "unsupported": H.ERR_UNSUPPORTED, "bad_block": H.ERR_BAD_BLOCK}
    assert [w for _, _, w in table].count("ok") == 1 and len(table) == 18
    for entry, (call, untouched, reads_boxes) in _entries(H).items():
        for name, blk, want in table:
            expect = STATUS[want] if reads_boxes or want != "unsupported" else CONTINUITY_ON_BOXES
            rc = call(blk)
            assert rc == expect, (entry, name, rc, L.hpsdf_last_error())
            if rc:
                assert L.hpsdf_last_error(), (entry, name)
                assert untouched(), (entry, name)
