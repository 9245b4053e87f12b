"""QueryBounds against Query on the same trees: hpsdf_query_bounds_device and hpsdf_query_bounds_grid_device over inputs resident in
HBM, union3 @ 1e-5 (every leaf in the top table) and union3 @ 1e-7, timed with HIP events on one context and one stream.

Inputs:
  boxes   1 M random boxes of edge 1/256 of the root, centres uniform in the root (48 bytes read a box)
  grid    the 256^3 cells of the root through the grid entry (no box array: nothing read)
each at subdiv 1, 2 and 4, max_leaves 4096.

Method (tools/bench_cast_rays.py's): every call is warmed up at the timed size (the first bounds call on a tree also builds its
constants; it is not timed); then WINDOWS windows per call, the calls alternating window by window, each window CALLS launches between
two events.  Reported per call: median, fastest and slowest window in us a launch.  A box costs one leaf evaluation -- what Query spends
on a point once it has found the leaf -- per sub-box of every leaf it reaches, so the yardstick is (mean evaluations a box) x (Query's
time a point, measured on as many uniform points in the same tree), with evaluations = leaves x subdiv^3 from the call's own out_leaves
(an upper bound: a leaf the walk passes without reaching it evaluates nothing).  The ratio says what the walk costs beyond its
evaluations -- the descent with a range, the stack in LDS -- or saves: Query's descent is paid once per leaf, not once per evaluation.

    python tools/bench_query_bounds.py [--boxes 1048576] [--grid 256] [--out profiles/query_bounds_timing]   (writes <out>.json and <out>.txt)
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

WINDOWS, CALLS, WARMUP = 5, 3, 1
MAX_LEAVES = 4096
SUBDIVS = (1, 2, 4)
STATUS = ("ok", "leaf limit", "invalid", "not finite")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bounds_timing"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import hpsdf_loader
    import oracle as O
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    nb, g = args.boxes, args.grid
    ng = g * g * g
    rng = np.random.default_rng(20261019)
    c = rng.uniform(-0.5 + 1.0 / 512, 0.5 - 1.0 / 512, (nb, 3))
    boxes_h = np.ascontiguousarray(np.concatenate([c - 1.0 / 512, c + 1.0 / 512], 1))
    stream = torch.cuda.Stream()
    results, lines = [], []
    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        boxes = torch.from_numpy(boxes_h).cuda()
        nmax = max(nb, ng)
        pts = torch.from_numpy(O.splitmix64_points(nmax)).cuda()
        lo = torch.empty(nmax, dtype=torch.float64, device="cuda")
        hi = torch.empty(nmax, dtype=torch.float64, device="cuda")
        status = torch.empty(nmax, dtype=torch.uint8, device="cuda")
        leaves = torch.empty(nmax, dtype=torch.int32, device="cuda")
        val = torch.empty(nmax, dtype=torch.float64, device="cuda")
        L = H.lib()
        vp = lambda a: C.c_void_p(a.data_ptr())
        lo3, hi3, n3 = (C.c_double * 3)(-0.5, -0.5, -0.5), (C.c_double * 3)(0.5, 0.5, 0.5), (C.c_uint32 * 3)(g, g, g)

        for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
            blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            calls = {}
            for sd in SUBDIVS:
                calls["boxes subdiv %d" % sd] = lambda sd=sd: H.check(L.hpsdf_query_bounds_device(
                    ctx.handle, tree.handle, vp(boxes), nb, sd, MAX_LEAVES, vp(lo), vp(hi), vp(status), vp(leaves)))
                calls["grid subdiv %d" % sd] = lambda sd=sd: H.check(L.hpsdf_query_bounds_grid_device(
                    ctx.handle, tree.handle, lo3, hi3, n3, sd, MAX_LEAVES, vp(lo), vp(hi), vp(status), vp(leaves)))
            calls["query boxes"] = lambda: H.check(L.hpsdf_query_device(ctx.handle, tree.handle, vp(pts), nb, vp(val)))
            calls["query grid"] = lambda: H.check(L.hpsdf_query_device(ctx.handle, tree.handle, vp(pts), ng, vp(val)))
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
            rec = {"tree": name, "boxes": nb, "grid": g, "max_degree": info["max_degree"], "max_depth": info["max_depth"],
                   "leaves": info["n_leaves"], "max_leaves": MAX_LEAVES, "windows": WINDOWS, "calls_per_window": CALLS, "us_per_launch": {},
                   "inputs": {}}
            for k, w in windows.items():
                count = nb if "boxes" in k else ng
                rec["us_per_launch"][k] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
                lines.append("%-14s %-16s median %12.1f us  (min %12.1f, max %12.1f)  %9.2f M a second"
                             % (name, k, statistics.median(w), min(w), max(w), count / statistics.median(w)))
            for k, call in calls.items():
                if k.startswith("query"):
                    continue
                kind, sd = k.split()[0], int(k.split()[-1])
                count = nb if kind == "boxes" else ng
                call()
                torch.cuda.synchronize()
                st = status[:count].cpu().numpy()
                lv = leaves[:count].cpu().numpy().view(np.uint32).astype(np.float64)
                l, h = lo[:count].cpu().numpy(), hi[:count].cpu().numpy()
                ok = st == 0
                decided = float(((l[ok] > 0) | (h[ok] < 0)).sum()) / count
                share = (np.bincount(st, minlength=4) / float(count)).tolist()
                ev = lv * sd ** 3
                wave = lv[:count - count % 64].reshape(-1, 64)
                q_us = rec["us_per_launch"]["query " + kind]["median"]
                us = rec["us_per_launch"][k]["median"]
                s = {"status_share": dict(zip(STATUS, share)), "mean_leaves": float(lv.mean()), "mean_evaluations": float(ev.mean()),
                     "mean_wave_max_leaves": float(wave.max(1).mean()), "decided_share": decided, "mean_width": float((h[ok] - l[ok]).mean()),
                     "yardstick_us": float(ev.mean()) * q_us}
                s["bounds_over_yardstick"] = us / s["yardstick_us"] if s["yardstick_us"] > 0 else None
                rec["inputs"][k] = s
                lines.append("%-14s %-16s status share %s; sign decided for %.4f of the boxes; mean width %.4g"
                             % (name, k, ", ".join("%s %.4f" % (a, b) for a, b in zip(STATUS, share)), decided, s["mean_width"]))
                lines.append("%-14s %-16s mean leaves a box %.3f (mean over waves of the largest %.2f), mean evaluations %.2f"
                             % (name, k, s["mean_leaves"], s["mean_wave_max_leaves"], s["mean_evaluations"]))
                lines.append("%-14s %-16s bounds / (mean evaluations x Query) = %.1f / (%.2f x %.1f) = %.3f"
                             % (name, k, us, s["mean_evaluations"], q_us, s["bounds_over_yardstick"] or 0.0))
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
