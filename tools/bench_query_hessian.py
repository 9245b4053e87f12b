"""QueryHessian against QueryGradient on the same trees and points: hpsdf_query_hessian_device (the Hessian alone; the Hessian and the
curvature) and hpsdf_query_true_gradient_device over 10 M seeded random points resident in HBM, union3 @ 1e-5 (every leaf of degree
<= 2 in the top table) and union3 @ 1e-7, timed with HIP events on one context and one stream, all in one process.

Method (that of tools/bench_query_gradient.py): every call is warmed up at the timed size; then WINDOWS windows per call, the calls
alternating window by window (other work shares the machine: alternating puts a drift into all of them), each window CALLS launches
between two events.  Reported per call: median, fastest and slowest window in us a launch, and the ratio of the medians to
QueryGradient's.  Bytes a point are counted, not measured: 24 read, then 8 + 24 written by QueryGradient, 48 by the Hessian alone and
48 + 16 with the curvature, plus the leaf's row.  No time here is a pass or fail condition: the call is new.

    python tools/bench_query_hessian.py [--points N] [--out profiles/query_hessian_timing]      (writes <out>.json and <out>.txt)
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
BYTES = {"query_hessian (hess)": 24 + 48, "query_hessian (hess + curv)": 24 + 48 + 16, "query_true_gradient": 24 + 8 + 24}   # without the leaf's row
BASE = "query_true_gradient"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_hessian_timing"))
    args = ap.parse_args()
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
        hess = torch.empty(6 * n, dtype=torch.float64, device="cuda")
        curv = torch.empty(2 * n, dtype=torch.float64, device="cuda")
        L = H.lib()
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            calls = {
                "query_hessian (hess)": lambda: H.check(L.hpsdf_query_hessian_device(ctx.handle, tree.handle, vp(pts), n, 0, None, None, vp(hess), None)),
                "query_hessian (hess + curv)": lambda: H.check(L.hpsdf_query_hessian_device(ctx.handle, tree.handle, vp(pts), n, 0, None, None, vp(hess),
                                                                                             vp(curv))),
                BASE: lambda: H.check(L.hpsdf_query_true_gradient_device(ctx.handle, tree.handle, vp(pts), n, 0, vp(out), vp(grad))),
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
                   "windows": WINDOWS, "calls_per_window": CALLS, "us_per_launch": {}, "over_query_gradient": {}, "bytes_per_point": BYTES}
            base = statistics.median(windows[BASE])
            for k, w in windows.items():
                med = statistics.median(w)
                rec["us_per_launch"][k] = {"median": med, "min": min(w), "max": max(w)}
                rec["over_query_gradient"][k] = med / base
                lines.append("%-14s %-28s median %8.1f us  (min %8.1f, max %8.1f)  %6.2f Gpts/s  %.3f x QueryGradient  %3d bytes a point"
                             % (name, k, med, min(w), max(w), n / med / 1e3, med / base, BYTES[k]))
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
