"""ClearanceBatch against a loop of Clearance on the trees of tools/bench_clearance.py -- union3 @ 1e-5 (A, the unit root) against
sphere075 @ 1e-6 (B, the root [-0.25, 5]^3) -- for n = 1, 16, 256 and 4096 random rigid poses (seed 2024: a random rotation, and a
translation that puts A's centre at a distance from B's centre drawn, a third each, from [0.2, 0.9] (interpenetrating), [1.0, 1.5]
(touching) and [1.8, 3.5] (apart), in a direction with positive components so that A stays inside B's root), at depth 10, tol 0,
max_leaves 256, on one context and one stream.

In the same run, alternating, REPEATS times each after one warm-up of every shape:
  * hpsdf_clearance_batch_device for the n poses                    (the new call)
  * a loop of n hpsdf_clearance_device calls over the same poses    (the existing code: the reference of the ratio)
and the batch again with decide = 1e-6 (B's iso: "do the solids touch", with a proof).  The entries synchronise before they return, so
a call is timed on the host clock around the call.  Every struct of the batch is compared with the loop's, byte for byte.

Reported per n: the medians and the spread in ms, loop / batch, the time per pose, the cells visited over all poses, the most levels of
a pose, the statuses, and how many poses ended apart (lo > iso_b), interpenetrating (hi < iso_b) and undecided.

    python tools/bench_clearance_batch.py [--out profiles/clearance_batch_timing] [--counts 1,16,256,4096]   (writes <out>.txt)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

REPEATS = 5          # of a case with 256 poses or more
SMALL_REPEATS = 50   # of a smaller one: a call is a fraction of a millisecond
COUNTS = (1, 16, 256, 4096)
DEPTH = 10
MAX_CELLS = 1 << 24
MAX_TOTAL = 1 << 28
MAX_LEAVES = 256
ISO_A, ISO_B = 1e-5, 1e-6
CENTRE_B = np.array((0.25, 0.0, 0.0))


def random_poses(H, n, seed=2024):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12))
    for i in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        lo, hi = ((0.2, 0.9), (1.0, 1.5), (1.8, 3.5))[i % 3]
        u = np.abs(rng.normal(size=3))
        out[i] = H.pose(q, CENTRE_B + rng.uniform(lo, hi) * u / np.linalg.norm(u))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_batch_timing"))
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    ap.add_argument("--depth", type=int, default=DEPTH)
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    import torch
    import hpsdf_loader
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    stream = torch.cuda.Stream()
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        blk_a, _ = H.create_block(ctx, H.make_config(1e-5), H.Field.union3(), 1024)
        blk_b, _ = H.create_block(ctx, H.make_config(1e-6, (-0.25,) * 3, (5.0,) * 3), H.Field.sphere((0.25, 0.0, 0.0), 0.75), 1024)
        ta, tb = H.DeviceTree(ctx, blk_a), H.DeviceTree(ctx, blk_b)
        say("A: union3 @ 1e-5 (%d leaves, max degree %d), iso_a %g; B: sphere075 @ 1e-6 (%d leaves, max degree %d); depth %d, tol 0, max_leaves %d, "
            "max_cells 2^24, max_total_cells 2^28; %d timed repeats (%d below 256 poses) after one warm-up, batch and loop alternating"
            % (ta.info()["n_leaves"], ta.info()["max_degree"], ISO_A, tb.info()["n_leaves"], tb.info()["max_degree"], args.depth, MAX_LEAVES, REPEATS, SMALL_REPEATS))
        shared = (ISO_A, args.depth, 0.0, MAX_CELLS, MAX_LEAVES)
        for n in counts:
            poses = random_poses(H, n)
            batch = lambda decide=None: ta.clearance_batch(tb, poses, *shared, decide=decide, max_total_cells=MAX_TOTAL)
            loop = lambda: [ta.clearance(tb, p, *shared) for p in poses]
            calls = {"batch": batch, "loop": loop, "batch, decide": lambda: batch(ISO_B)}
            res = {k: f() for k, f in calls.items()}                             # the warm-up of every shape
            ms = {k: [] for k in calls}
            for _ in range(REPEATS if n >= 256 else SMALL_REPEATS):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    res[k] = f()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            same = res["batch"].raw == b"".join(r.raw for r in res["loop"])
            med = {k: statistics.median(v) for k, v in ms.items()}
            for k in calls:
                say("n %5d  %-14s median %11.3f ms (min %11.3f, max %11.3f)  %9.4f ms a pose" % (n, k, med[k], min(ms[k]), max(ms[k]), med[k] / n))
            say("n %5d  loop / batch = %.2f; loop / (batch, decide) = %.2f; the batch's structs %s the loop's" % (n, med["loop"] / med["batch"],
                                                                                                                   med["loop"] / med["batch, decide"],
                                                                                                                   "equal" if same else "DIFFER FROM"))
            for k in ("batch", "batch, decide"):
                r = res[k]
                say("n %5d  %-14s %d cells visited, at most %d levels, statuses %s; %d apart, %d interpenetrating, %d undecided"
                    % (n, k, int(r.cells_visited.sum()), int(r.levels.max()) + 1, {int(s): int(c) for s, c in zip(*np.unique(r.status, return_counts=True))},
                       int((r.lo > ISO_B).sum()), int((r.hi < ISO_B).sum()), int(((r.lo <= ISO_B) & (r.hi >= ISO_B)).sum())))
            if not same:
                raise SystemExit("the batch differs from the loop: no timing of it is worth anything")
        ta.close(), tb.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
