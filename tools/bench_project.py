"""ProjectToSurface against QueryGradient on the same trees: hpsdf_project_device (tol 1e-9, 16 steps) and
hpsdf_query_true_gradient_device over 10 M seeded random points resident in HBM, union3 @ 1e-5 (every leaf in the top table) and
union3 @ 1e-7, timed with HIP events on one context and one stream.

Method (tools/bench_query_gradient.py's): every call is warmed up at the timed size; then WINDOWS windows per call, the calls
alternating window by window (other work shares the machine: alternating puts a drift into all of them), each window CALLS launches
between two events.  Reported per call: median, fastest and slowest window in us a launch.  A projection costs one field evaluation --
one QueryGradient -- per step and one more where it stops, so the yardstick is (mean evaluations a point) x (QueryGradient's time),
with the evaluations counted from the call's own out_iters (iters + 1); the ratio to it says what the loop costs beyond its
evaluations: lanes that have stopped idle until the last lane of their wave has.

    python tools/bench_project.py [--points N] [--out profiles/project_timing]      (writes <out>.json and <out>.txt)
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

WINDOWS, CALLS, WARMUP = 9, 20, 3
TOL, MAX_ITER = 1e-9, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_timing"))
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
        oxyz = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        grad = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        iters = torch.empty(n, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        L = H.lib()
        vp = lambda t: C.c_void_p(t.data_ptr())
        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            calls = {
                "project": lambda: H.check(L.hpsdf_project_device(ctx.handle, tree.handle, vp(pts), n, 0.0, TOL, MAX_ITER, 0, vp(oxyz), vp(out), vp(grad),
                                                                  vp(iters), vp(status))),
                "project (points only)": lambda: H.check(L.hpsdf_project_device(ctx.handle, tree.handle, vp(pts), n, 0.0, TOL, MAX_ITER, 0, vp(oxyz), None,
                                                                                None, None, None)),
                "query_true_gradient": lambda: H.check(L.hpsdf_query_true_gradient_device(ctx.handle, tree.handle, vp(pts), n, 0, vp(out), vp(grad))),
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
            calls["project"]()
            torch.cuda.synchronize()
            it, st = iters.cpu().numpy(), status.cpu().numpy()
            evals = it.astype(np.float64) + 1.0
            # what a wave costs: its slowest point's evaluations (64 consecutive points a wave)
            wave = evals[:n - n % 64].reshape(-1, 64)
            rec = {"tree": name, "points": n, "max_degree": info["max_degree"], "max_depth": info["max_depth"], "leaves": info["n_leaves"],
                   "tol": TOL, "max_iter": MAX_ITER, "windows": WINDOWS, "calls_per_window": CALLS, "us_per_launch": {},
                   "status_counts": np.bincount(st, minlength=4).tolist(), "iters_histogram": np.bincount(it, minlength=MAX_ITER + 1).tolist(),
                   "mean_evaluations": float(evals.mean()), "mean_wave_max_evaluations": float(wave.max(1).mean()) if len(wave) else None}
            for k, w in windows.items():
                rec["us_per_launch"][k] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
                lines.append("%-14s %-24s median %9.1f us  (min %9.1f, max %9.1f)  %6.2f Gpts/s" % (name, k, statistics.median(w), min(w), max(w),
                                                                                                  n / statistics.median(w) / 1e3))
            qg = rec["us_per_launch"]["query_true_gradient"]["median"]
            rec["yardstick_us"] = rec["mean_evaluations"] * qg
            rec["project_over_yardstick"] = rec["us_per_launch"]["project"]["median"] / rec["yardstick_us"]
            lines.append("%-14s status counts (converged, iteration limit, left root, flat) %s" % (name, rec["status_counts"]))
            lines.append("%-14s mean evaluations a point %.3f (iters + 1); mean over waves of the slowest lane's %.3f"
                         % (name, rec["mean_evaluations"], rec["mean_wave_max_evaluations"] or 0.0))
            lines.append("%-14s project / (mean evaluations x QueryGradient) = %.1f / (%.3f x %.1f) = %.3f"
                         % (name, rec["us_per_launch"]["project"]["median"], rec["mean_evaluations"], qg, rec["project_over_yardstick"]))
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
