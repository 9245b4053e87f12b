"""IntegratePair on union3 @ 1e-5 (A, the unit root) against sphere075 @ 1e-6 (B, the root [-0.25, 5]^3) under a rotated pose:
hpsdf_integrate_pair_device for the intersection, the union and the difference at depth 8, 10 and 12 with 2 samples per axis, on one
context and one stream -- and, in the same run, the two things a level is made of:

  * hpsdf_integrate_device on A at the same depth: the cost of the levels without B;
  * hpsdf_query_bounds_device on B over the image boxes of the call's FINAL cells (subdiv 1, the call's max_leaves, with the `leaves`
    output): the cost of the walks alone, and how many leaves of B a walk passes.

The two entries synchronise before they return, so a call is timed on the host clock around the call (bench_integrate.py has why); every
case is warmed up once and then timed CALLS times.  QueryBounds is timed with HIP events.  The image boxes are made here, with torch,
from the cell array by the header's statements without the slack; QueryBounds refuses a box that leaves B's root where IntegratePair
clamps it, so the boxes are clipped to B's root and those that miss it are left out (they cost the call no walk either).  Boxes are
walked for every final cell, also where A alone decided the cell and the call did not walk; the lists before the last are not walked
again here.  The boxes go through QueryBounds in runs of 2^22 cells in list order (a launch of fewer measures the launch); above WALK_CELLS final
cells evenly spaced runs are timed and the time is scaled to the whole.

Reported per case: the call's median, fastest and slowest time in ms; the final cells by class and the evaluations of A; Integrate's
median; the walks' time, the boxes walked, the mean leaves a walk and the mean over waves of the largest walk's leaves (a wave costs its
slowest lane); and the ratio of the call to (Integrate + walks).

    python tools/bench_integrate_pair.py [--out profiles/integrate_pair_timing]   (writes <out>.txt)
"""
import argparse
import ctypes as C
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
SAMPLES = 2
MAX_CELLS = 1 << 28
MAX_LEAVES = 256
WALK_CELLS = 1 << 26
RUN = 1 << 22
OPS = ("intersection", "union", "difference")


def rotated_pose(H):
    a = np.array((0.3, -0.5, 0.8)) / np.linalg.norm((0.3, -0.5, 0.8))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return H.pose(np.eye(3) + math.sin(0.6) * K + (1 - math.cos(0.6)) * (K @ K), (0.6, 0.3, 0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrate_pair_timing"))
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

    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        L = H.lib()
        vp = lambda a: C.c_void_p(a.data_ptr())
        blk_a, _ = H.create_block(ctx, H.make_config(1e-5), H.Field.union3(), 1024)
        blk_b, _ = H.create_block(ctx, H.make_config(1e-6, (-0.25,) * 3, (5.0,) * 3), H.Field.sphere((0.25, 0.0, 0.0), 0.75), 1024)
        ta, tb = H.DeviceTree(ctx, blk_a), H.DeviceTree(ctx, blk_b)
        pose = rotated_pose(H)
        P = torch.from_numpy(pose.reshape(3, 4)).cuda()
        M, t = P[:, :3].contiguous(), P[:, 3].contiguous()
        b_lo, b_hi = torch.full((3,), -0.25, dtype=torch.float64, device="cuda"), torch.full((3,), 5.0, dtype=torch.float64, device="cuda")
        say("A: union3 @ 1e-5 (%d leaves, max degree %d); B: sphere075 @ 1e-6 (%d leaves, max degree %d); pose: rotation by 0.6 rad about "
            "(0.3, -0.5, 0.8), translation (0.6, 0.3, 0.3); %d samples per axis, max_leaves %d"
            % (ta.info()["n_leaves"], ta.info()["max_degree"], tb.info()["n_leaves"], tb.info()["max_degree"], SAMPLES, MAX_LEAVES))

        def host_clock(call):
            res = call()
            ms = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                res = call()
                ms.append((time.perf_counter() - t0) * 1e3)
            return res, ms

        def walks(cells):
            """QueryBounds of B over the image boxes of `cells` -> (ms scaled to all cells, boxes walked scaled, mean leaves a walk,
            mean over waves of the largest walk's leaves, share of the cells measured)"""
            n = len(cells)
            runs = [(s, min(s + RUN, n)) for s in range(0, n, RUN)]
            if n > WALK_CELLS:
                runs = runs[::int(math.ceil(n / WALK_CELLS))]
            total_ms, boxes_n, leaves_sum, wave_sum, wave_n, measured = 0.0, 0, 0, 0.0, 0, 0
            for s, e in runs:
                raw = torch.from_numpy(cells[s:e].view(np.uint8).reshape(-1, 12)).cuda().to(torch.int64)
                depth = raw[:, 4]
                ijk = torch.stack([raw[:, 6] | (raw[:, 7] << 8), raw[:, 8] | (raw[:, 9] << 8), raw[:, 10] | (raw[:, 11] << 8)], 1).to(torch.float64)
                sz = torch.ldexp(torch.ones_like(depth, dtype=torch.float64), -depth)[:, None]
                cx = (-0.5 + ijk * sz) + 0.5 * sz                                  # A's root is the unit cube centred at 0: x = p
                hx = 0.5 * sz.expand(-1, 3)
                yc = cx @ M.T + t
                r = hx @ M.abs().T
                lo, hi = torch.maximum(yc - r, b_lo), torch.minimum(yc + r, b_hi)
                keep = (lo <= hi).all(1)
                boxes = torch.cat([lo[keep], hi[keep]], 1).contiguous()
                m = len(boxes)
                measured += e - s
                if m == 0:
                    continue
                out_lo, out_hi = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
                status, leaves = torch.empty(m, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")
                call = lambda: H.check(L.hpsdf_query_bounds_device(ctx.handle, tb.handle, vp(boxes), m, 1, MAX_LEAVES, vp(out_lo), vp(out_hi),
                                                                   vp(status), vp(leaves)))
                call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                torch.cuda.synchronize()
                total_ms += e0.elapsed_time(e1)
                boxes_n += m
                leaves_sum += int(leaves.sum())
                whole = leaves[:m - m % 64].reshape(-1, 64)
                wave_sum += float(whole.max(1).values.sum())
                wave_n += len(whole)
            scale = n / max(measured, 1)
            return total_ms * scale, int(boxes_n * scale), leaves_sum / max(boxes_n, 1), wave_sum / max(wave_n, 1), measured / max(n, 1)

        for depth in depths:
            one, ms_one = host_clock(lambda: ta.integrate(1e-5, depth, SAMPLES, MAX_CELLS))
            say("depth %2d  Integrate(A): median %9.3f ms (min %9.3f, max %9.3f), %d final cells, %d evaluations"
                % (depth, statistics.median(ms_one), min(ms_one), max(ms_one), one.cells_inside + one.cells_outside + one.cells_undecided,
                   one.evaluations))
            for op, name in enumerate(OPS):
                res, ms = host_clock(lambda: ta.integrate_pair(tb, op, pose, 1e-5, 1e-6, depth, SAMPLES, MAX_CELLS, MAX_LEAVES))
                cells = ta.integrate_pair(tb, op, pose, 1e-5, 1e-6, depth, SAMPLES, MAX_CELLS, MAX_LEAVES, cells=True).cells
                walk_ms, boxes, mean_leaves, wave_leaves, share = walks(cells)
                del cells
                med = statistics.median(ms)
                say("depth %2d  %-12s median %9.3f ms (min %9.3f, max %9.3f)  status %d, %d levels" % (depth, name, med, min(ms), max(ms), res.status, res.levels))
                say("depth %2d  %-12s %d final cells (%d inside, %d outside, %d undecided), %d evaluations of A, unit volume in [%.9f, %.9f]"
                    % (depth, name, res.cells_inside + res.cells_outside + res.cells_undecided, res.cells_inside, res.cells_outside,
                       res.cells_undecided, res.evaluations, res.unit_volume_lo, res.unit_volume_hi))
                say("depth %2d  %-12s walks of B over the final cells' boxes: %9.3f ms for %d boxes (%.0f %% of the cells timed), %.2f leaves a "
                    "walk, %.2f the largest of a wave" % (depth, name, walk_ms, boxes, 100 * share, mean_leaves, wave_leaves))
                say("depth %2d  %-12s call / (Integrate + walks) = %.3f / (%.3f + %.3f) ms = %.2f"
                    % (depth, name, med, statistics.median(ms_one), walk_ms, med / (statistics.median(ms_one) + walk_ms)))
        ta.close(), tb.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
