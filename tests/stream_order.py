"""What tests/test_gpu_stream_order.py is made of: a calibrated delay on a stream, input sets that are all valid but all different, the
device entries as (inputs, outputs, call) triples, and a step that loads its inputs, calls, clones and overwrites on one stream with no
host wait -- then says WHICH wrong answer came back when the clone is not the synchronised call's.

The idea: every input buffer holds a valid set P0 before anything is queued, the real set P1 arrives by a device-to-device copy behind a
delay, and a third valid set P2 overwrites it right after the call.  A launch on another stream, or a host-side step that does not wait
for the right one, then computes P0's or P2's answer, or leaves the outputs' 7.0 fill: well-defined, and wrong.  Nothing here can read
or write outside a buffer whatever order the work runs in."""
import ctypes as C
import gc

import numpy as np
import torch

FILL = 7
F64, U8, U16, U32 = torch.float64, torch.uint8, torch.int16, torch.int32   # (16- and 32-bit outputs are compared as bytes: the sign is moot)
DELAY_MS = (50.0, 100.0)


# ------------------------------------------------------------------------------------------------------------ the delay
class Delay:
    """Device work that keeps a stream busy for 50-100 ms, measured with events on the machine the test runs on: torch.cuda._sleep
    with a calibrated cycle count, or (where that is missing or does not spin) a calibrated chain of matrix products."""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.kind, self.count, self.ms = None, 0, 0.0
        target = 0.5 * (DELAY_MS[0] + DELAY_MS[1])
        for kind, first in (("sleep", 20_000_000), ("matmul", 8)):
            if kind == "sleep" and not hasattr(torch.cuda, "_sleep"):
                continue
            if kind == "matmul":
                self.a = torch.ones((4096, 4096), device="cuda")
                self.b = torch.empty_like(self.a)
            self.kind = kind
            self._measure(first)                                             # (the first launch pays for the kernel's load)
            count, ms = first, self._measure(first)
            for _ in range(3):
                if ms <= 0.01:
                    break
                count = max(1, int(round(count * target / ms)))
                ms = self._measure(count)
                if DELAY_MS[0] <= ms <= DELAY_MS[1]:
                    self.count, self.ms = count, ms
                    return
        raise AssertionError("no delay of %g-%g ms could be calibrated (last: %s x %d = %.3f ms)" % (DELAY_MS + (self.kind, count, ms)))

    def _work(self, count):
        if self.kind == "sleep":
            torch.cuda._sleep(int(count))
        else:
            for _ in range(int(count)):
                torch.mm(self.a, self.a, out=self.b)

    def _measure(self, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            self._work(count)
            e1.record()
        self.stream.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self):
        """The delay on the current stream -> an event recorded right behind it (event.query() is False while the delay runs)."""
        self._work(self.count)
        ev = torch.cuda.Event()
        ev.record()
        return ev


class quiet_host:
    """The sequence under test is the only thing this thread does while it is queued: Python's collector is run first and held off
    inside.  A collection in the middle of it can finalise trees, contexts and tensors of earlier tests, and freeing device memory waits
    for the device -- the delay included -- which the no-host-wait assertions would then lay at the entry's door."""

    def __enter__(self):
        gc.collect()
        torch.cuda.synchronize()
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *a):
        if self.was:
            gc.enable()


# ------------------------------------------------------------------------------------------------------------ input sets
def points(rng, n):
    """strictly inside the root [-0.5, 0.5]^3"""
    return (rng.uniform(-0.49, 0.49, (n, 3)),)


def boxes(rng, n):
    """inside the root, a few leaves wide"""
    lo = rng.uniform(-0.45, 0.3, (n, 3))
    return (np.concatenate([lo, lo + rng.uniform(0.01, 0.12, (n, 3))], 1),)


def rays(rng, n):
    """from a corner region of the root that union3 leaves empty, to a point well inside its sphere (centre (-0.2, -0.15, 0.1), radius
    0.18) reached at t = 1: the field changes sign on every ray"""
    o = np.stack([rng.uniform(-0.45, -0.42, n), rng.uniform(0.3, 0.45, n), rng.uniform(0.3, 0.45, n)], 1)
    target = np.array([-0.2, -0.15, 0.1]) + rng.uniform(-0.03, 0.03, (n, 3))
    return o, target - o, np.ones(n)


def three_sets(make, n, seed):
    """P0, P1, P2: three draws of one construction"""
    return [make(np.random.default_rng(seed + k), n) for k in range(3)]


# ------------------------------------------------------------------------------------------------------------ the entries
def _p(t):
    return t.data_ptr()


class Entry:
    """make(rng, n) -> the input arrays; outputs(n) -> [(shape, dtype)]; call(H, ctx, obj, ins, outs, n) queues the entry on ctx's stream
    (obj: the DeviceTree uploaded through ctx, or the field); asynchronous: the header promises no host wait."""

    def __init__(self, make, outputs, call, asynchronous=True):
        self.make, self.outputs, self.call, self.asynchronous = make, outputs, call, asynchronous


def _query(H, ctx, tree, ins, outs, n):
    H.check(H.lib().hpsdf_query_device(ctx.handle, tree.handle, C.c_void_p(_p(ins[0])), n, C.c_void_p(_p(outs[0]))))


def _query_with_gradient(H, ctx, tree, ins, outs, n):
    H.check(H.lib().hpsdf_query_gradient_device(ctx.handle, tree.handle, C.c_void_p(_p(ins[0])), n, C.c_void_p(_p(outs[0])),
                                                C.c_void_p(_p(outs[1]))))


def _field_eval(H, ctx, field, ins, outs, n):
    H.check(H.lib().hpsdf_field_eval_device(ctx.handle, field.handle, C.c_void_p(_p(ins[0])), n, C.c_void_p(_p(outs[0]))))


GRID_LO, GRID_HI, GRID_N = (-0.45, -0.4, -0.35), (0.4, 0.45, 0.3), (15, 20, 10)   # 3 000 cells


ENTRIES = {
    "query": Entry(points, lambda n: [((n,), F64)], _query),
    "query_with_gradient": Entry(points, lambda n: [((n,), F64), ((n, 3), F64)], _query_with_gradient),
    "query_gradient": Entry(points, lambda n: [((n,), F64), ((n, 3), F64)],
                            lambda H, ctx, t, i, o, n: t.query_gradient_device(_p(i[0]), n, _p(o[0]), _p(o[1]))),
    "query_hessian": Entry(points, lambda n: [((n,), F64), ((n, 3), F64), ((n, 6), F64), ((n, 2), F64)],
                           lambda H, ctx, t, i, o, n: t.query_hessian_device(_p(i[0]), n, *[_p(x) for x in o])),
    "project": Entry(points, lambda n: [((n, 3), F64), ((n,), F64), ((n, 3), F64), ((n,), U8), ((n,), U8)],
                     lambda H, ctx, t, i, o, n: t.project_device(_p(i[0]), n, *[_p(x) for x in o])),
    "cast_rays": Entry(rays, lambda n: [((n,), U8), ((n,), F64), ((n, 3), F64), ((n,), F64), ((n, 3), F64), ((n,), U16), ((n,), U16)],
                       lambda H, ctx, t, i, o, n: t.cast_rays_device(_p(i[0]), _p(i[1]), _p(i[2]), n, *[_p(x) for x in o])),
    "query_bounds": Entry(boxes, lambda n: [((n,), F64), ((n,), F64), ((n,), U8), ((n,), U32)],
                          lambda H, ctx, t, i, o, n: t.query_bounds_device(_p(i[0]), n, *[_p(x) for x in o])),
    # (the lattice is three host triples: no device input, so only the outputs' fill can show)
    "query_bounds_grid": Entry(lambda rng, n: (), lambda n: [((n,), F64), ((n,), F64), ((n,), U8), ((n,), U32)],
                               lambda H, ctx, t, i, o, n: t.query_bounds_grid_device(GRID_LO, GRID_HI, GRID_N, *[_p(x) for x in o])),
    "field_eval": Entry(points, lambda n: [((n,), F64)], _field_eval),
}


# ------------------------------------------------------------------------------------------------------------ one call in stream order
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fill(entry, n):
    return [torch.full(shape, FILL, dtype=dt, device="cuda") for shape, dt in entry.outputs(n)]


def synchronised(H, ctx, entry, obj, sets, n):
    """The entry called the ordinary way for each input set: inputs complete before the call, outputs read after a full
    synchronisation -> per set, the outputs as numpy arrays."""
    out = []
    for s in sets:
        ins, outs = [_dev(a) for a in s], _fill(entry, n)
        torch.cuda.synchronize()
        entry.call(H, ctx, obj, ins, outs, n)
        ctx.synchronize()
        torch.cuda.synchronize()
        out.append([o.cpu().numpy() for o in outs])
    if sets[0]:   # the three answers have to differ, or a stale one could not be told from the right one
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert any(x.tobytes() != y.tobytes() for x, y in zip(out[a], out[b])), "P%d and P%d give one answer" % (a, b)
    return out


class Step:
    """One call of an entry inside a sequence on one stream.  The buffers are made here (inputs hold P0, outputs the fill) and must be
    complete before anything is queued: torch.cuda.synchronize() after the last Step is built.  load(), call(), clone() and overwrite()
    queue on the CURRENT torch stream and on ctx's stream, which the test keeps the same; none of them waits."""

    def __init__(self, H, ctx, entry, obj, sets, n):
        self.H, self.ctx, self.entry, self.obj, self.n = H, ctx, entry, obj, n
        self.ins = [_dev(a) for a in sets[0]]
        self.p1 = [_dev(a) for a in sets[1]]
        self.p2 = [_dev(a) for a in sets[2]]
        self.outs = _fill(entry, n)
        self.got = None

    def load(self):
        for d, s in zip(self.ins, self.p1):
            d.copy_(s, non_blocking=True)

    def call(self):
        self.entry.call(self.H, self.ctx, self.obj, self.ins, self.outs, self.n)

    def clone(self):
        self.got = [o.clone() for o in self.outs]

    def overwrite(self):
        for d, s in zip(self.ins, self.p2):
            d.copy_(s, non_blocking=True)

    def check(self, refs, what):
        """after the stream has been synchronised: the clones against the synchronised call's outputs for P1, byte for byte"""
        got = [g.cpu().numpy() for g in self.got]
        wrong = [describe(k, g, [r[k] for r in refs]) for k, g in enumerate(got) if g.tobytes() != refs[1][k].tobytes()]
        assert not wrong, "%s: %s" % (what, "; ".join(wrong))


def _rows(a):
    return np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint8)


def describe(k, got, refs):
    """which wrong answer output k holds: P0's (inputs read too early), P2's (too late), the fill (outputs written too late)"""
    fill = np.full_like(got, FILL)
    names = (("P0's answer: the inputs were read too early", refs[0]), ("P2's answer: the inputs were read too late", refs[2]),
             ("the %d fill: the outputs were written too late, or on another stream" % FILL, fill))
    for name, r in names:
        if got.tobytes() == r.tobytes():
            return "output %d is %s" % (k, name)
    g = _rows(got)
    count = lambda r: int((g == _rows(r)).all(1).sum())
    return ("output %d is a mixture over its %d rows: %d equal P1's answer, %d P0's (read too early), %d P2's (read too late), %d the fill "
            "(written too late)" % (k, len(g), count(refs[1]), count(refs[0]), count(refs[2]), count(fill)))


def run_pattern(H, ctx, S, delay, entry, obj, sets, n):
    """delay, P1 -> inputs, the entry, a clone of the outputs, P2 -> inputs: all on S, no host wait -> (the step, whether the delay was
    still running when the entry returned).  S is synchronised before this returns."""
    step = Step(H, ctx, entry, obj, sets, n)
    with quiet_host(), torch.cuda.stream(S):
        ev = delay.enqueue()
        step.load()
        step.call()
        pending = not ev.query()
        step.clone()
        step.overwrite()
    S.synchronize()
    return step, pending
