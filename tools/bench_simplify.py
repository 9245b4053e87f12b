"""Times Simplify (include/hpsdf.h, "Simplify") on the device and on the calling thread, on the same blocks, and writes
profiles/simplify_timing.txt:

    python tools/bench_simplify.py [--repeats 5] [--no-mesh] [--out profiles/simplify_timing.txt]

Trees: the product's union3 @ 1e-7 and sphere @ 1e-8, and the largest mesh tree bench.py --full builds (the displaced torus grid of
2 097 152 triangles at targetError 1e-6, root = the mesh's box + 0.02).  rms 1e-4, 1e-3 and 1e-2.  Per case: the median wall time of
hpsdf_simplify (block in host memory in, block in host memory out: uploads, the level loop, downloads and the host-side assembly are all
inside) and of hpsdf_simplify_block, and the counts in and out.  The two return the same bytes; that is asserted for every case."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-mesh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import hpsdf_loader
    H = hpsdf_loader.load()
    from helpers import displaced_torus, product_field
    ctx = H.Context(0)
    trees = [("union3 @ 1e-7", H.create_block(ctx, H.make_config(1e-7), product_field(H, "union3"), 1024)[0]),
             ("sphere @ 1e-8", H.create_block(ctx, H.make_config(1e-8), product_field(H, "sphere"), 1024)[0])]
    if not args.no_mesh:
        verts, tris = displaced_torus()
        lo, hi = verts.min(0) - 0.02, verts.max(0) + 0.02
        field = H.Field.mesh(ctx, verts, tris)
        trees.append(("torus mesh (2 097 152 triangles) @ 1e-6", H.create_block(ctx, H.make_config(1e-6, tuple(lo), tuple(hi)), field, 1024)[0]))
        field.close()
    lines = ["Simplify: hpsdf_simplify (device) against hpsdf_simplify_block (calling thread), same block, same bytes out",
             "median of %d calls after one warm-up, wall time of the whole call, ms" % args.repeats, "",
             "%-42s %6s %9s %9s %9s %9s %7s %6s %10s %10s" % ("tree", "rms", "nodes in", "coeffs in", "nodes out", "coeffs out", "merges", "levels",
                                                             "device ms", "host ms")]
    for name, blk in trees:
        for rms in (1e-4, 1e-3, 1e-2):
            dev, st = H.simplify(ctx, blk, rms)
            host, hst = H.simplify_block(blk, rms)
            assert dev == host and st == hst, (name, rms)
            d_ms = median_ms(lambda: H.simplify(ctx, blk, rms), args.repeats)
            h_ms = median_ms(lambda: H.simplify_block(blk, rms), args.repeats)
            lines.append("%-42s %6g %9d %9d %9d %9d %7d %6d %10.3f %10.3f" % (name, rms, st["nodes_in"], st["coeffs_in"], st["nodes_out"], st["coeffs_out"],
                                                                             st["merges"], st["levels"], d_ms, h_ms))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
