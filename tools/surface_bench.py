"""hpsdf_extract_surface on union3 @ 1e-5 (every leaf in the top table) and @ 1e-7 (the general path) over the root box at n = 256 and
512 cubes per axis: device ms of each phase (hpsdf_surface_last_timings: lattice values, counts, scans, output, download) and the
lattice pass's rate next to hpsdf_query_device on the same lattice points materialised as an array in HBM.  Prints one JSON line.
    usage: python tools/surface_bench.py [--reps R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hpsdf_loader  # noqa: E402

H = hpsdf_loader.load()


def lattice_points_device(lo, hi, n):
    """The lattice points of include/hpsdf.h on the device, L order: lo + (f64)i * h, the product and the sum as separate operations."""
    cols = []
    for a in range(3):
        h = (hi[a] - lo[a]) / n[a]
        cols.append((torch.arange(n[a] + 1, dtype=torch.float64, device="cuda") * h) + lo[a])
    N0, N1, N2 = n[0] + 1, n[1] + 1, n[2] + 1
    pts = torch.empty((N2, N1, N0, 3), dtype=torch.float64, device="cuda")
    pts[..., 0] = cols[0][None, None, :]
    pts[..., 1] = cols[1][None, :, None]
    pts[..., 2] = cols[2][:, None, None]
    return pts.reshape(-1, 3)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    stream = torch.cuda.Stream()
    rows = []
    with torch.cuda.stream(stream):
        ctx = H.Context(0, stream.cuda_stream)
        for target in (1e-5, 1e-7):
            blk, st = H.create_block(ctx, H.make_config(target), H.Field.union3(), 0)
            tree = H.DeviceTree(ctx, blk)
            info = tree.info()
            for n in (256, 512):
                lo, hi, n3 = (-0.5,) * 3, (0.5,) * 3, (n, n, n)
                npts = (n + 1) ** 3
                phases, walls = [], []
                for r in range(reps + 1):
                    t0 = time.perf_counter()
                    verts, tris = tree.extract_surface(lo, hi, n3)
                    w = (time.perf_counter() - t0) * 1e3
                    if r:  # the first call is a warm-up
                        phases.append(H.surface_last_timings())
                        walls.append(w)
                med = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
                # the same points through Query, materialised in HBM (24 B a point read, 8 B written)
                pts = lattice_points_device(lo, hi, n3)
                out = torch.empty(npts, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                tree.query_device(pts.data_ptr(), npts, out.data_ptr())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    tree.query_device(pts.data_ptr(), npts, out.data_ptr())
                e1.record(stream)
                e1.synchronize()
                q_ms = e0.elapsed_time(e1) / reps
                # the extraction's own values for the same points (bitwise, as the tests require)
                _, _, vals = tree.extract_surface(lo, hi, n3, values=True)
                same = bool(np.array_equal(vals.ravel().view(np.uint64), out.cpu().numpy().view(np.uint64)))
                del pts, out
                device_ms = med["lattice"] + med["count"] + med["scan"] + med["emit"]
                rows.append({
                    "tree": "union3@%g" % target, "n_nodes": info["n_nodes"], "max_depth": info["max_depth"],
                    "max_degree": info["max_degree"], "n": n, "lattice_points": npts, "verts": len(verts), "tris": len(tris),
                    "ms": {k: round(v, 4) for k, v in med.items()}, "device_pipeline_ms": round(device_ms, 4),
                    "wall_ms": round(float(np.median(walls)), 3),
                    "lattice_gpts_s": round(npts / med["lattice"] / 1e6, 3) if med["lattice"] > 0 else None,
                    "query_materialised_ms": round(q_ms, 4), "query_materialised_gpts_s": round(npts / q_ms / 1e6, 3),
                    "lattice_values_equal_query": same,
                })
                print(json.dumps(rows[-1]), file=sys.stderr)
            tree.close()
        ctx.close()
    print(json.dumps({"tool": "surface_bench", "device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}))


if __name__ == "__main__":
    main()
