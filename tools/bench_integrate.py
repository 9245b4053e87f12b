"""Integrate on union3 @ 1e-5 (every leaf in the top table) and union3 @ 1e-7: hpsdf_integrate_device at depth 8, 10 and 12 with 2
samples per axis, on one context and one stream.

hpsdf_integrate_device synchronises before it returns (it reads one count per level back to size the next list), so a call is timed on
the host clock around the call: what a caller waits for -- the kernels, the scans, the per-level round trips and the allocations.
Every case is warmed up once (the first call on a tree also builds its constants and its list 0; it is not timed), then CALLS calls are
timed one by one.  Reported per case: median, fastest and slowest call in ms; the final cells by class; the polynomial evaluations; the
width unit_volume_hi - unit_volume_lo; and the ratio of the call's time to evaluations x (Query's time a point, measured with HIP
events on POINTS uniform points in the same tree) -- what the refinement costs beyond its evaluations.  Beside depth 8 stands the
lattice of the same cell width through hpsdf_query_bounds_grid_device (256^3 cells, subdiv 1, HIP events); the lattices of depth 10 and
12 (2^30 and 2^36 cells) are not run: the first needs 18 GB of outputs, the second is out of the entry's range.

    python tools/bench_integrate.py [--out profiles/integrate_timing]   (writes <out>.json and <out>.txt)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CALLS = 5
DEPTHS = (8, 10, 12)
SAMPLES = 2
MAX_CELLS = 1 << 28
POINTS = 1 << 22
GRID = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrate_timing"))
    args = ap.parse_args()
    import torch
    import hpsdf_loader
    import oracle as O
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    stream = torch.cuda.Stream()
    results, lines = [], []
    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        L = H.lib()
        vp = lambda a: C.c_void_p(a.data_ptr())
        pts = torch.from_numpy(O.splitmix64_points(POINTS)).cuda()
        val = torch.empty(POINTS, dtype=torch.float64, device="cuda")
        ng = GRID ** 3
        lo = torch.empty(ng, dtype=torch.float64, device="cuda")
        hi = torch.empty(ng, dtype=torch.float64, device="cuda")
        status = torch.empty(ng, dtype=torch.uint8, device="cuda")
        lo3, hi3, n3 = (C.c_double * 3)(-0.5, -0.5, -0.5), (C.c_double * 3)(0.5, 0.5, 0.5), (C.c_uint32 * 3)(GRID, GRID, GRID)

        def events(call, repeat):
            call()
            torch.cuda.synchronize()
            out = []
            for _ in range(repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1))
            return statistics.median(out)

        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            query_ms = events(lambda: H.check(L.hpsdf_query_device(ctx.handle, tree.handle, vp(pts), POINTS, vp(val))), CALLS)
            ns_point = query_ms * 1e6 / POINTS
            rec = {"tree": name, "max_degree": info["max_degree"], "max_depth": info["max_depth"], "leaves": info["n_leaves"],
                   "samples": SAMPLES, "max_cells": MAX_CELLS, "query_ns_a_point": ns_point, "cases": {}}
            lines.append("%-14s Query: %.3f ns a point (%d points)" % (name, ns_point, POINTS))
            for depth in DEPTHS:
                tree.integrate(0.0, depth, SAMPLES, MAX_CELLS)
                ms = []
                for _ in range(CALLS):
                    t0 = time.perf_counter()
                    res = tree.integrate(0.0, depth, SAMPLES, MAX_CELLS)
                    ms.append((time.perf_counter() - t0) * 1e3)
                cells = res.cells_inside + res.cells_outside + res.cells_undecided
                width = res.unit_volume_hi - res.unit_volume_lo
                yard = res.evaluations * ns_point * 1e-6
                rec["cases"]["depth %d" % depth] = {
                    "ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}, "status": res.status, "levels": res.levels,
                    "cells": cells, "cells_inside": res.cells_inside, "cells_outside": res.cells_outside, "cells_undecided": res.cells_undecided,
                    "evaluations": res.evaluations, "unit_volume_lo": res.unit_volume_lo, "unit_volume_hi": res.unit_volume_hi,
                    "unit_volume": res.unit_volume, "width": width, "yardstick_ms": yard, "integrate_over_yardstick": statistics.median(ms) / yard}
                lines.append("%-14s depth %2d  median %9.3f ms (min %9.3f, max %9.3f)  status %d, %d levels" % (name, depth, statistics.median(ms), min(ms), max(ms), res.status, res.levels))
                lines.append("%-14s depth %2d  %d final cells (%d inside, %d outside, %d undecided), %d evaluations"
                             % (name, depth, cells, res.cells_inside, res.cells_outside, res.cells_undecided, res.evaluations))
                lines.append("%-14s depth %2d  unit volume in [%.12f, %.12f], width %.3e, estimate %.12f"
                             % (name, depth, res.unit_volume_lo, res.unit_volume_hi, width, res.unit_volume))
                lines.append("%-14s depth %2d  integrate / (evaluations x Query) = %.3f / %.3f ms = %.2f" % (name, depth, statistics.median(ms), yard, statistics.median(ms) / yard))
            grid_ms = events(lambda: H.check(L.hpsdf_query_bounds_grid_device(ctx.handle, tree.handle, lo3, hi3, n3, 1, 4096, vp(lo), vp(hi), vp(status), None)), CALLS)
            l, h = lo.cpu().numpy(), hi.cpu().numpy()
            und = float(((l <= 0.0) & (h >= 0.0)).sum()) / ng
            rec["query_bounds_grid_256"] = {"ms": grid_ms, "undecided_volume": und}
            lines.append("%-14s QueryBoundsGrid %d^3 (the lattice of depth 8's width): %.3f ms; undecided volume %.3e" % (name, GRID, grid_ms, und))
            results.append(rec)
            tree.close()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    with open(args.out + ".txt", "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
