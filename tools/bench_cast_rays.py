"""CastRays against QueryGradient on the same trees: hpsdf_cast_rays_device (tol 1e-9, the default limits) over ray sets resident in
HBM, union3 @ 1e-5 (every leaf in the top table) and union3 @ 1e-7, timed with HIP events on one context and one stream.

Ray sets, 1 M rays each (|d| = 1, t_max 10):
  camera   a 1024 x 1024 orthographic grid seen from outside the root, the view tilted off the axes; row-major, so neighbouring lanes are
           neighbouring pixels
  random   origins on a sphere around the root, aimed at uniform points inside it
  inside   origins uniform inside the root, uniform directions -- the set hpsdf_query_ray_device is also timed on, for orientation only
           (it is the reference's sphere tracing: another question, answered to a fixed 1e-4)

Method (tools/bench_project.py's): every call is warmed up at the timed size; then WINDOWS windows per call, the calls alternating window
by window, each window CALLS launches between two events.  Reported per call: median, fastest and slowest window in us a launch.  A
cast costs one field evaluation -- one QueryGradient -- per sample and per refinement step, so the yardstick is (mean evaluations a
ray) x (QueryGradient's time a point, measured on as many uniform points in the same tree), with the evaluations taken from the call's
own out_evals; the ratio to it says what the walk costs beyond its evaluations: the descents per leaf, and lanes that have stopped
idling until the last lane of their wave has.

    python tools/bench_cast_rays.py [--side 1024] [--out profiles/cast_rays_timing]      (writes <out>.json and <out>.txt)
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

WINDOWS, CALLS, WARMUP = 7, 5, 2
TOL, MAX_ITER, MAX_CELLS, T_MAX = 1e-9, 32, 4096, 10.0
STATUS = ("hit", "miss", "unconverged", "cell limit", "invalid")


def ray_sets(np, side):
    n = side * side
    view = np.array([0.35, -0.22, -1.0])
    view /= np.linalg.norm(view)
    right = np.cross(view, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, view)
    px = (np.arange(side) + 0.5) / side - 0.5
    u, v = np.meshgrid(px, px)
    cam_o = -2.0 * view[None, :] + 1.2 * (u.reshape(-1, 1) * right[None, :] + v.reshape(-1, 1) * up[None, :])
    cam_d = np.ascontiguousarray(np.broadcast_to(view, cam_o.shape))
    rng = np.random.default_rng(20261018)
    w = rng.normal(size=(n, 3))
    ro = 1.5 * w / np.linalg.norm(w, axis=1, keepdims=True)
    rd = rng.uniform(-0.45, 0.45, (n, 3)) - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    io = rng.uniform(-0.49, 0.49, (n, 3))
    idir = rng.normal(size=(n, 3))
    idir /= np.linalg.norm(idir, axis=1, keepdims=True)
    return {"camera": (cam_o, cam_d), "random": (ro, rd), "inside": (io, idir)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast_rays_timing"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import hpsdf_loader
    import oracle as O
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n = args.side * args.side
    stream = torch.cuda.Stream()
    results, lines = [], []
    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        sets = {k: tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in v) for k, v in ray_sets(np, args.side).items()}
        tmax = torch.full((n,), T_MAX, dtype=torch.float64, device="cuda")
        pts = torch.from_numpy(O.splitmix64_points(n)).cuda()
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        xyz = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        val = torch.empty(n, dtype=torch.float64, device="cuda")
        grad = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        evals = torch.empty(n, dtype=torch.int16, device="cuda")
        cells = torch.empty(n, dtype=torch.int16, device="cuda")
        hit = torch.empty(n, dtype=torch.uint8, device="cuda")
        L = H.lib()
        vp = lambda a: C.c_void_p(a.data_ptr())

        def cast(o, d):
            H.check(L.hpsdf_cast_rays_device(ctx.handle, tree.handle, vp(o), vp(d), vp(tmax), n, 0.0, TOL, MAX_ITER, MAX_CELLS, 0, vp(status),
                                             vp(t), vp(xyz), vp(val), vp(grad), vp(evals), vp(cells)))

        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            calls = {"cast " + k: (lambda o=o, d=d: cast(o, d)) for k, (o, d) in sets.items()}
            calls["query_ray inside"] = lambda: H.check(L.hpsdf_query_ray_device(ctx.handle, tree.handle, vp(sets["inside"][0]),
                                                                                  vp(sets["inside"][1]), vp(tmax), n, vp(hit), vp(t)))
            calls["query_true_gradient"] = lambda: H.check(L.hpsdf_query_true_gradient_device(ctx.handle, tree.handle, vp(pts), n, 0, vp(val),
                                                                                             vp(grad)))
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
            rec = {"tree": name, "rays": n, "max_degree": info["max_degree"], "max_depth": info["max_depth"], "leaves": info["n_leaves"],
                   "tol": TOL, "max_iter": MAX_ITER, "max_cells": MAX_CELLS, "windows": WINDOWS, "calls_per_window": CALLS, "us_per_launch": {},
                   "sets": {}}
            for k, w in windows.items():
                rec["us_per_launch"][k] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
                lines.append("%-14s %-22s median %10.1f us  (min %10.1f, max %10.1f)  %8.2f M a second" % (name, k, statistics.median(w), min(w), max(w),
                                                                                                           n / statistics.median(w)))
            qg = rec["us_per_launch"]["query_true_gradient"]["median"]
            for k, (o, d) in sets.items():
                cast(o, d)
                torch.cuda.synchronize()
                st = status.cpu().numpy()
                ev = evals.cpu().numpy().view(np.uint16).astype(np.float64)
                ce = cells.cpu().numpy().view(np.uint16).astype(np.float64)
                wave = ev[:n - n % 64].reshape(-1, 64)
                share = (np.bincount(st, minlength=5) / float(n)).tolist()
                us = rec["us_per_launch"]["cast " + k]["median"]
                s = {"status_share": dict(zip(STATUS, share)), "mean_evaluations": float(ev.mean()), "mean_cells": float(ce.mean()),
                     "mean_wave_max_evaluations": float(wave.max(1).mean()), "yardstick_us": float(ev.mean()) * qg}
                s["cast_over_yardstick"] = us / s["yardstick_us"] if s["yardstick_us"] > 0 else None
                rec["sets"][k] = s
                lines.append("%-14s %-8s status share %s" % (name, k, ", ".join("%s %.4f" % (a, b) for a, b in zip(STATUS, share))))
                lines.append("%-14s %-8s mean evaluations a ray %.2f, mean cells %.2f; mean over waves of the slowest lane's evaluations %.2f"
                             % (name, k, s["mean_evaluations"], s["mean_cells"], s["mean_wave_max_evaluations"]))
                lines.append("%-14s %-8s cast / (mean evaluations x QueryGradient) = %.1f / (%.2f x %.1f) = %.3f"
                             % (name, k, us, s["mean_evaluations"], qg, s["cast_over_yardstick"] or 0.0))
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
