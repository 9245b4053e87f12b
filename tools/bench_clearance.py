"""Clearance on union3 @ 1e-5 (A, the unit root) against sphere075 @ 1e-6 (B, the root [-0.25, 5]^3): hpsdf_clearance_device at depth 8,
10 and 12 (tol 0, max_leaves 256) under three poses, on one context and one stream --

  * rotated:          tools/bench_integrate_pair.py's pose (A's root across B's surface and across the low faces of B's root);
  * separated:        a translation by (3, 3, 3): A's solid well outside B's, a positive clearance;
  * interpenetrating: a translation by (0.55, 0.3, 0.3): A's root around B's centre, a negative clearance;

and, in the same run, the yardsticks: hpsdf_integrate_pair_device for the intersection under the same pose at the same depth (2 samples
per axis) -- the call that answered "do they touch" before -- and hpsdf_clearance_host, the same search on the calling thread.  The
entries synchronise before they return, so a call is timed on the host clock around the call; every case is warmed up once and then
timed CALLS times.

Reported per case: the median, fastest and slowest time in ms; the enclosure [lo, hi] and its width; the status and the levels; the
cells visited, dropped by A's class, pruned and left open; IntegratePair's and the calling thread's median and the ratios.

    python tools/bench_clearance.py [--out profiles/clearance_timing]   (writes <out>.txt)
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CALLS = 5
DEPTHS = (8, 10, 12)
MAX_CELLS = 1 << 28
MAX_LEAVES = 256


def rotated_pose(H):
    a = np.array((0.3, -0.5, 0.8)) / np.linalg.norm((0.3, -0.5, 0.8))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return H.pose(np.eye(3) + math.sin(0.6) * K + (1 - math.cos(0.6)) * (K @ K), (0.6, 0.3, 0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_timing"))
    ap.add_argument("--depths", default=",".join(str(d) for d in DEPTHS))
    args = ap.parse_args()
    depths = [int(d) for d in args.depths.split(",")]
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

    def host_clock(call):
        res = call()
        ms = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            res = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return res, ms

    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        blk_a, _ = H.create_block(ctx, H.make_config(1e-5), H.Field.union3(), 1024)
        blk_b, _ = H.create_block(ctx, H.make_config(1e-6, (-0.25,) * 3, (5.0,) * 3), H.Field.sphere((0.25, 0.0, 0.0), 0.75), 1024)
        ta, tb = H.DeviceTree(ctx, blk_a), H.DeviceTree(ctx, blk_b)
        say("A: union3 @ 1e-5 (%d leaves, max degree %d), iso_a 1e-5; B: sphere075 @ 1e-6 (%d leaves, max degree %d); tol 0, max_leaves %d; "
            "IntegratePair: the intersection, iso_b 1e-6, 2 samples per axis" % (ta.info()["n_leaves"], ta.info()["max_degree"], tb.info()["n_leaves"],
                                                                                 tb.info()["max_degree"], MAX_LEAVES))
        poses = (("rotated", rotated_pose(H)), ("separated", H.pose(None, (3.0, 3.0, 3.0))), ("interpenetrating", H.pose(None, (0.55, 0.3, 0.3))))
        for name, pose in poses:
            for depth in depths:
                res, ms = host_clock(lambda: ta.clearance(tb, pose, 1e-5, depth, 0.0, MAX_CELLS, MAX_LEAVES))
                _, ms_host = host_clock(lambda: ta.clearance(tb, pose, 1e-5, depth, 0.0, MAX_CELLS, MAX_LEAVES, host=True))
                pair, ms_pair = host_clock(lambda: ta.integrate_pair(tb, H.PAIR_INTERSECTION, pose, 1e-5, 1e-6, depth, 2, MAX_CELLS, MAX_LEAVES))
                med, med_host, med_pair = statistics.median(ms), statistics.median(ms_host), statistics.median(ms_pair)
                say("%-16s depth %2d  Clearance median %9.3f ms (min %9.3f, max %9.3f)  status %d, %d levels, min in [%.9g, %.9g] (width %.3g)"
                    % (name, depth, med, min(ms), max(ms), res.status, res.levels, res.lo, res.hi, res.hi - res.lo))
                say("%-16s depth %2d  %d cells visited, %d outside A, %d pruned, %d open" % (name, depth, res.cells_visited, res.cells_outside_a,
                                                                                          res.cells_pruned, res.cells_open))
                say("%-16s depth %2d  IntegratePair median %9.3f ms (%d final cells, volume in [%.6g, %.6g]): Clearance / IntegratePair = %.3f"
                    % (name, depth, med_pair, pair.cells_inside + pair.cells_outside + pair.cells_undecided, pair.volume_lo, pair.volume_hi, med / med_pair))
                say("%-16s depth %2d  on the calling thread median %9.3f ms: device / calling thread = %.2f" % (name, depth, med_host, med / med_host))
        ta.close(), tb.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
