"""QueryGradient against QueryWithGradient on the same trees: hpsdf_query_true_gradient_device and hpsdf_query_gradient_device over
10 M seeded random points resident in HBM, union3 @ 1e-5 (every leaf in the top table) and union3 @ 1e-7, timed with HIP events on
one context and one stream.

Method: both calls are warmed up at the timed size; then WINDOWS windows per call, the two calls alternating window by window (other
work shares the machine: alternating puts a drift into both), each window CALLS launches between two events.  Reported per call:
median, fastest and slowest window in us a launch.  Bytes a point are counted, not measured: 24 read + 8 + 24 written for both calls
(QueryWithGradient leaves rows of outside points unwritten; the random points are all inside), plus the leaf's row.

    python tools/bench_query_gradient.py [--points N] [--out profiles/query_gradient_timing]      (writes <out>.json and <out>.txt)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WINDOWS, CALLS, WARMUP = 9, 40, 5
BYTES_TRUE = 24 + 8 + 24       # per point, without the leaf's row
BYTES_SHORTCUT = 24 + 8 + 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_gradient_timing"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import hpsdf_loader
    import oracle as O
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n = args.points
    stream = torch.cuda.Stream()
    results, lines = [], []
    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        pts = torch.from_numpy(O.splitmix64_points(n)).cuda()
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        grad = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        L = H.lib()
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            calls = {
                "query_true_gradient": lambda: H.check(L.hpsdf_query_true_gradient_device(ctx.handle, tree.handle, vp(pts), n, 0, vp(out), vp(grad))),
                "query_true_gradient_unit": lambda: H.check(L.hpsdf_query_true_gradient_device(ctx.handle, tree.handle, vp(pts), n, 1, vp(out), vp(grad))),
                "query_gradient (shortcut)": lambda: H.check(L.hpsdf_query_gradient_device(ctx.handle, tree.handle, vp(pts), n, vp(out), vp(grad))),
            }
            for call in calls.values():
                for _ in range(WARMUP):
                    call()
            torch.cuda.synchronize()
            windows = {k: [] for k in calls}
            for _ in range(WINDOWS):
                for k, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(CALLS):
                        call()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    windows[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            rec = {"tree": name, "points": n, "max_degree": info["max_degree"], "max_depth": info["max_depth"], "leaves": info["n_leaves"],
                   "windows": WINDOWS, "calls_per_window": CALLS, "us_per_launch": {}}
            for k, w in windows.items():
                rec["us_per_launch"][k] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
                lines.append("%-14s %-28s median %8.1f us  (min %8.1f, max %8.1f)  %6.1f Gpts/s" % (name, k, statistics.median(w), min(w), max(w),
                                                                                                  n / statistics.median(w) / 1e3))
            rec["true_over_shortcut"] = rec["us_per_launch"]["query_true_gradient_unit"]["median"] / rec["us_per_launch"]["query_gradient (shortcut)"]["median"]
            rec["bytes_per_point"] = {"query_true_gradient": BYTES_TRUE, "query_gradient (shortcut)": BYTES_SHORTCUT, "ratio": BYTES_TRUE / BYTES_SHORTCUT}
            lines.append("%-14s unit QueryGradient / QueryWithGradient = %.3f in time, %.3f in bytes a point (%d / %d, the leaf's row apart)"
                         % (name, rec["true_over_shortcut"], BYTES_TRUE / BYTES_SHORTCUT, BYTES_TRUE, BYTES_SHORTCUT))
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
