#!/usr/bin/env python3
"""Points per second of the K-nearest point queries (rt_closest_points with the options "closest_k" / "closest_all") beside the default
closest-point call, in one process.

Points: bench_closest.py's `--grid`^3 grid (128: 2.1 M points) over the configuration's bounding box, unbounded (R = +inf) and in the
narrow band (R = two cell widths).  After a warm-up the forms are timed alternately, `--repeats` times each: median [min .. max].  All
through the device entry on torch tensors, torch events around the call (it includes the origin-bound reduction).

  default        K = 1, all = 0: k_closest, today's call
  K = 4, K = 8   the list, pruned by the K-th key
  K = 1, all     the closest point plus the overlap count: bounded by R alone.  Unbounded it examines every primitive for every point,
                 so that one form runs on every `--all-stride`-th point only (default 64) and its time is per point examined

One more call of each form runs the counting kernel (option "closest_count") for the node steps and primitive tests per point.

    python tools/bench_nearest.py --config 3
"""
import argparse
import json
import os
import statistics
import sys

import torch  # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = (("default", 1, 0), ("K = 4", 4, 0), ("K = 8", 8, 0), ("K = 1, all", 1, 1))


def summary(ms, items):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "points": items,
            "mitems_per_s": round(items / med * 1e-3, 1)}


def torch_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 5])
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--all-stride", type=int, default=64)
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    corners = np.concatenate([np.asarray(tris[k]).reshape(-1, 3) for k in ("posA", "posB", "posC")])
    lo, hi = corners.min(0), corners.max(0)
    G = args.grid
    axes = [np.linspace(lo[a], hi[a], G, dtype=np.float32) for a in range(3)]
    cell = float(max((hi - lo) / (G - 1)))
    n = G ** 3
    pts = np.zeros((n, 8), np.float32)
    pts[:, 0:3] = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    pts[:, 3] = np.inf
    rows, counts = {}, {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        free = torch.from_numpy(pts).cuda()
        band = free.clone()
        band[:, 3] = 2.0 * cell
        sparse = free[::args.all_stride].contiguous()

        def form(k, count_all, points):
            def run():
                t.set_option("closest_k", k)
                t.set_option("closest_all", count_all)
                try:
                    return t.closest_points(points)
                finally:
                    t.set_option("closest_k", 1)
                    t.set_option("closest_all", 0)
            return run
        forms = []
        for where, points in (("unbounded", free), (f"R = 2 cells ({2 * cell:.4g})", band)):
            for name, k, count_all in FORMS:
                p = sparse if (count_all and points is free) else points
                forms.append((f"{name}, {where}", form(k, count_all, p), int(p.shape[0]), k))
        for _, fn, _, _ in forms:
            fn()                                                                   # warm-up of every form
        ms = {name: [] for name, _, _, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn, _, _ in forms:
                ms[name].append(torch_time(fn))
        for name, _, items, _ in forms:
            rows[name] = summary(ms[name], items)
        t.set_option("closest_count", 1)
        for name, fn, items, k in forms:
            res = fn().reshape(items, k, 16)
            info = t.closest_info()
            counts[name] = {"node_steps_per_point": round(info["lastNodeSteps"] / items, 2), "prim_tests_per_point": round(info["lastPrimTests"] / items, 2),
                            "found": int((res[:, 0, 7].view(torch.int32) != 0).sum().item()),
                            "mean_count": round(float(res[:, 0, 14].contiguous().view(torch.int32).double().mean().item()), 2)}
        t.set_option("closest_count", 0)
        st = t.stats()

    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {G}^3 = {n} points, cell {cell:.4g}, {args.repeats} repeats")
    for name, s in rows.items():
        print(f"  {name:40s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['points']:8d} points {s['mitems_per_s']:9.1f} M/s")
    for name, c in counts.items():
        print(f"  {name:40s} {c['node_steps_per_point']:9.2f} node steps, {c['prim_tests_per_point']:10.2f} primitive tests per point, {c['found']} found, mean count {c['mean_count']}")
    print(json.dumps({"config": args.config, "grid": G, "points": n, "cell": cell, "repeats": args.repeats, "rows": rows, "counts": counts}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
