"""ExtractSurfaceDual on union3 @ 1e-5 (every leaf in the top table) and union3 @ 1e-7 over a 256^3 lattice of the root: the phase
times of hpsdf_extract_surface_dual (hpsdf_surface_dual_last_timings: events on the context stream), V, T and the number of Hermite
evaluations (one per crossing edge: marching cubes' vertex count on the same lattice), beside hpsdf_extract_surface on the same
lattice, tree and context (hpsdf_surface_last_timings) and the ratio of the two whole-call times.  Marching cubes' kernels are the ones
the commit before this call was added had: surface.hip's device code is unchanged by it.

Every call is warmed up once, then CALLS calls are timed; the medians are reported.

    python tools/bench_surface_dual.py [--out profiles/surface_dual_timing.txt] [--n 256]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = 5
DUAL_PHASES = ("lattice", "ballots", "scan", "hermite", "vertices", "quads", "d2h", "total")
MC_PHASES = ("lattice", "count", "scan", "emit", "d2h", "total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_dual_timing.txt"))
    ap.add_argument("--n", type=int, default=256)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hpsdf_loader
    H = hpsdf_loader.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    ctx = H.Context(0)
    lo, hi, n = (-0.5,) * 3, (0.5,) * 3, (args.n,) * 3
    lines = ["%s, lattice %d^3 over the root, tau 0.1, medians of %d calls after one warm-up, device milliseconds" % (torch.cuda.get_device_name(0), args.n, CALLS)]
    for name, target in (("union3 @ 1e-5", 1e-5), ("union3 @ 1e-7", 1e-7)):
        blk, _ = H.create_block(ctx, H.make_config(target), H.Field.union3(), 1024)
        tree = H.DeviceTree(ctx, blk)
        info = tree.info()
        dual, mc = [], []
        for i in range(CALLS + 1):
            verts, tris, inf = tree.extract_surface_dual(lo, hi, n, 0.0, 0.1, info=True)
            if i:
                dual.append(H.surface_dual_last_timings())
        for i in range(CALLS + 1):
            mv, mt = tree.extract_surface(lo, hi, n, 0.0)
            if i:
                mc.append(H.surface_last_timings())
        d = {k: statistics.median(x[k] for x in dual) for k in DUAL_PHASES}
        m = {k: statistics.median(x[k] for x in mc) for k in MC_PHASES}
        lines.append("%s (max degree %d, %d leaves)" % (name, info["max_degree"], info["n_leaves"]))
        lines.append("  dual contouring : V %d  T %d  Hermite evaluations %d (%.4f of the %d lattice points)  ranks 0..3: %s  clamped %d"
                     % (len(verts), len(tris), len(mv), len(mv) / float((args.n + 1) ** 3), (args.n + 1) ** 3,
                        np.bincount(inf & 3, minlength=4).tolist(), int(((inf & 4) != 0).sum())))
        lines.append("                    " + "  ".join("%s %.3f" % (k, d[k]) for k in DUAL_PHASES))
        lines.append("  marching cubes  : V %d  T %d" % (len(mv), len(mt)))
        lines.append("                    " + "  ".join("%s %.3f" % (k, m[k]) for k in MC_PHASES))
        lines.append("  dual / marching cubes, whole call: %.3f   (without the lattice values, which both compute alike: %.3f)"
                     % (d["total"] / m["total"], (d["total"] - d["lattice"]) / (m["total"] - m["lattice"])))
        tree.close()
    ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
