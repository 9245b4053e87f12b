"""hpsdf_extract_surface_sparse next to hpsdf_extract_surface on union3 @ 1e-5 and @ 1e-7 over the root box: dense and sparse,
alternating, at n = 256, 512 and 1000 cubes per axis (the dense call's range), sparse alone at 2048 and 4096.  Per run: medians over
the repetitions of the call's wall time (it ends in a device synchronise and the download) and of the device milliseconds of each
phase (hpsdf_surface_last_timings / the sparse call's stats), the active share of the blocks, peak device scratch, output sizes, and
whether the two calls' arrays are equal.  Writes profiles/surface_sparse.json and prints the same JSON line.
    usage: python tools/surface_sparse_bench.py [--reps R] [--max-n N] [--out PATH] [--targets 1e-5,1e-7]   (the trees, in this order)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import hpsdf_loader  # noqa: E402

H = hpsdf_loader.load()
LO, HI = (-0.5,) * 3, (0.5,) * 3
DENSE_N = (256, 512, 1000)
SPARSE_ONLY_N = (2048, 4096)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def median(rows):
    return {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}


def main():
    reps, max_n = max(arg("--reps", 10), 1), arg("--max-n", 4096)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "surface_sparse.json"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("surface_sparse_bench: no GPU (nothing is measured without one)")
    ctx = H.Context(0)
    rows = []
    for target in [float(x) for x in arg("--targets", "1e-5,1e-7").split(",")]:
        blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 0)
        tree = H.DeviceTree(ctx, blk)
        info = tree.info()
        for n in DENSE_N + SPARSE_ONLY_N:
            if n > max_n:
                continue
            n3 = (n, n, n)
            dense = n in DENSE_N
            d_wall, d_ms, s_wall, s_stats = [], [], [], []
            equal = None
            for r in range(reps + 1):  # the first round is the warm-up of both; the two calls alternate
                if dense:
                    t0 = time.perf_counter()
                    dv, dt = tree.extract_surface(LO, HI, n3)
                    w = (time.perf_counter() - t0) * 1e3
                    if r:
                        d_wall.append(w)
                        d_ms.append(H.surface_last_timings())
                t0 = time.perf_counter()
                sv, st, stats = tree.extract_surface_sparse(LO, HI, n3, stats=True)
                w = (time.perf_counter() - t0) * 1e3
                if r:
                    s_wall.append(w)
                    s_stats.append(stats)
                if dense and r == 0:
                    equal = bool(sv.tobytes() == dv.tobytes() and st.tobytes() == dt.tobytes())
                n_verts, n_tris = len(sv), len(st)
                del sv, st
                if dense:
                    del dv, dt
            sm = median([{k: v for k, v in s.items() if k.endswith("_ms")} for s in s_stats])
            row = {
                "tree": "union3@%g" % target, "n_nodes": info["n_nodes"], "max_depth": info["max_depth"], "max_degree": info["max_degree"],
                "n": n, "lattice_points": (n + 1) ** 3, "reps": reps, "verts": n_verts, "tris": n_tris,
                "blocks": s_stats[0]["blocks"], "active_blocks": s_stats[0]["active_blocks"],
                "active_share": round(s_stats[0]["active_blocks"] / s_stats[0]["blocks"], 5),
                "leaves_visited_per_block": round(s_stats[0]["leaves_visited"] / s_stats[0]["blocks"], 3),
                "sparse_peak_scratch_bytes": s_stats[0]["peak_scratch_bytes"],
                "sparse_ms": sm, "sparse_wall_ms": round(float(np.median(s_wall)), 3),
                "sparse_wall_ms_min_max": [round(min(s_wall), 3), round(max(s_wall), 3)],
            }
            if dense:
                dm = median(d_ms)
                row.update({
                    "dense_ms": dm, "dense_wall_ms": round(float(np.median(d_wall)), 3),
                    "dense_wall_ms_min_max": [round(min(d_wall), 3), round(max(d_wall), 3)],
                    "dense_scratch_bytes_formula": 8 * (n + 1) ** 3 + 20 * ((3 * (n + 1) ** 3 + 63) // 64) + 12 * ((n ** 3 + 63) // 64),
                    "device_ms_dense_over_sparse": round(dm["total"] / sm["total_ms"], 3) if sm["total_ms"] > 0 else None,
                    "wall_dense_over_sparse": round(float(np.median(d_wall)) / float(np.median(s_wall)), 3),
                    "arrays_equal": equal,
                })
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        tree.close()
    ctx.close()
    doc = {"tool": "surface_sparse_bench", "device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
