#!/usr/bin/env python3
"""Points per second of a closest-point query (rt_closest_points) beside a closest-hit ray query of the same size, in one process.

Points: a `--grid`^3 grid (128: 2.1 M points) over the configuration's bounding box — the cells a signed-distance bake fills.  After a
warm-up the forms are timed alternately, `--repeats` times each: median [min .. max].  All through the device entries on torch tensors,
torch events around the call (it includes the origin-bound reduction).

  closest, unbounded         R = +inf: every point finds its surface
  closest, R = 2 cells       R = two cell widths: the narrow band a bake keeps; most points miss
  rays, rt_trace_rays        the yardstick: as many resident rays from the grid points along (0.8, 0.36, 0.48), closest hit

One more call of each closest form runs the counting kernel (option "closest_count") for the node steps and primitive tests per point.

    python tools/bench_closest.py --config 3
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


def summary(ms, items):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mitems_per_s": round(items / med * 1e-3, 1)}


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
    pts[:, 4:7] = np.array([0.8, 0.36, 0.48], np.float32)                          # (read by the ray yardstick only; no axis-parallel component)
    rows, counts = {}, {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        free = torch.from_numpy(pts).cuda()
        band = free.clone()
        band[:, 3] = 2.0 * cell
        forms = (("closest, unbounded", lambda: t.closest_points(free)), (f"closest, R = 2 cells ({2 * cell:.4g})", lambda: t.closest_points(band)),
                 ("rays, rt_trace_rays", lambda: t.trace_rays(free)))
        for _, fn in forms:
            fn()                                                                   # warm-up of every form
        ms = {name: [] for name, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn in forms:
                ms[name].append(torch_time(fn))
        for name, _ in forms:
            rows[name] = summary(ms[name], n)
        t.set_option("closest_count", 1)
        for name, fn in forms[:2]:
            res = fn()
            info = t.closest_info()
            counts[name] = {"node_steps_per_point": round(info["lastNodeSteps"] / n, 2), "prim_tests_per_point": round(info["lastPrimTests"] / n, 2),
                            "found": int((res[:, 7].view(torch.int32) != 0).sum().item())}
        t.set_option("closest_count", 0)
        st = t.stats()

    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {G}^3 = {n} points, cell {cell:.4g}, {args.repeats} repeats")
    for name, s in rows.items():
        print(f"  {name:40s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mitems_per_s']:9.1f} M/s")
    for name, c in counts.items():
        print(f"  {name:40s} {c['node_steps_per_point']:8.2f} node steps, {c['prim_tests_per_point']:8.2f} primitive tests per point, {c['found']} of {n} found")
    print(json.dumps({"config": args.config, "grid": G, "points": n, "cell": cell, "repeats": args.repeats, "rows": rows, "counts": counts}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
