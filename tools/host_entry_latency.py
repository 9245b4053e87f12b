"""Latency of the *_host entries of the point and ray calls (hpsdf_query_host, hpsdf_query_gradient_host, hpsdf_query_true_gradient_host,
hpsdf_query_hessian_host, hpsdf_project_host, hpsdf_cast_rays_host, hpsdf_query_ray_host) through ctypes, every output asked for, at row
counts on each path of a host call: answered on the calling thread (1, 32), zero-copy or staged through the pinned buffer (33, 256, 4133),
staged or direct (20000).  Per entry and size: WINDOWS windows of 400 / 100 / 40 calls, median, fastest and slowest window in us a call
(about 3 us of it is the ctypes call).  HPSDF_LIBRARY=<name> times lib/libhpsdf_<name>.so, as everywhere.

    python tools/host_entry_latency.py
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import hpsdf_loader

WINDOWS = 9
H = hpsdf_loader.load()
ctx = H.Context(0)
blk, _ = H.create_block(ctx, H.make_config(1e-5), H.Field.union3(), 1024)
tree = H.DeviceTree(ctx, blk)
L = H.lib()
vp = lambda a: a.ctypes.data_as(C.c_void_p)
rng = np.random.default_rng(0)
for n in (1, 32, 33, 256, 4133, 20000):
    pts = rng.uniform(-0.5, 0.5, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    tm = np.full(n, 10.0)
    out, val, grad, hess, curv = np.empty(n), np.empty(n), np.empty((n, 3)), np.empty((n, 6)), np.empty((n, 2))
    xyz, it, st = np.empty((n, 3)), np.empty(n, np.uint8), np.empty(n, np.uint8)
    ev, ce = np.empty(n, np.uint16), np.empty(n, np.uint16)
    c, t = ctx.handle, tree.handle
    calls = {
        "query_host": lambda: L.hpsdf_query_host(c, t, vp(pts), n, vp(out)),
        "query_gradient_host": lambda: L.hpsdf_query_gradient_host(c, t, vp(pts), n, vp(out), vp(grad)),
        "query_true_gradient_host": lambda: L.hpsdf_query_true_gradient_host(c, t, vp(pts), n, 0, vp(out), vp(grad)),
        "query_hessian_host": lambda: L.hpsdf_query_hessian_host(c, t, vp(pts), n, 0, vp(out), vp(grad), vp(hess), vp(curv)),
        "project_host": lambda: L.hpsdf_project_host(c, t, vp(pts), n, 0.0, 1e-9, 16, 0, vp(xyz), vp(out), vp(grad), vp(it), vp(st)),
        "cast_rays_host": lambda: L.hpsdf_cast_rays_host(c, t, vp(pts), vp(d), vp(tm), n, 0.0, 1e-9, 32, 4096, 0, vp(st), vp(out), vp(xyz), vp(val),
                                                         vp(grad), vp(ev), vp(ce)),
        "query_ray_host": lambda: L.hpsdf_query_ray_host(c, t, vp(pts), vp(d), vp(tm), n, vp(st), vp(out)),
    }
    reps = 400 if n <= 32 else (100 if n <= 4133 else 40)
    for name, call in calls.items():
        assert call() == 0, name
        call()
        w = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            w.append((time.perf_counter() - t0) / reps * 1e6)
        print("%-26s n=%6d: median %9.2f us  min %9.2f  max %9.2f" % (name, n, statistics.median(w), min(w), max(w)), flush=True)
