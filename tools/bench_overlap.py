#!/usr/bin/env python3
"""Boxes per second of the box overlap queries (rt_closest_points with the option "closest_box") beside the K-nearest queries a caller
would otherwise use, in one process.

Boxes: bench_closest.py's `--grid`^3 grid (128: 2.1 M points) over the configuration's bounding box, each point the centre of a box of
half-extents cell / 2 — the grid's own cells, conservative voxelisation.  The yardstick: the K-nearest query of the same centres with
R = the cell's half-diagonal, the smallest ball that holds the box.  After a warm-up the forms are timed alternately, `--repeats` times
each: median [min .. max].  All through the device entry on torch tensors, torch events around the call (it includes the origin-bound
reduction).

  box (1, 0)     CheckBox: is there anything in the cell          sphere (1, 0)   the default closest-point call with R
  box (1, 1)     the voxel's count and its nearest surface         sphere (1, 1)   the overlap count within R
  box (4, 0), (8, 0)   the nearest 4 / 8 surfaces in the cell      sphere (4, 0), (8, 0)

One more call of each form runs the counting kernel (option "closest_count") for the node steps and primitive tests per box.

    python tools/bench_overlap.py --config 3
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

FORMS = ((1, 0), (1, 1), (4, 0), (8, 0))


def summary(ms, items):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "boxes": items,
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
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    corners = np.concatenate([np.asarray(tris[k]).reshape(-1, 3) for k in ("posA", "posB", "posC")])
    lo, hi = corners.min(0), corners.max(0)
    G = args.grid
    axes = [np.linspace(lo[a], hi[a], G, dtype=np.float32) for a in range(3)]
    cell = ((hi - lo) / (G - 1)).astype(np.float32)
    half = cell * np.float32(0.5)
    radius = float(np.linalg.norm(half))
    n = G ** 3
    pts = np.zeros((n, 8), np.float32)
    pts[:, 0:3] = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    rows, counts = {}, {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        boxes = torch.from_numpy(pts).cuda()
        boxes[:, 3] = 1.0
        boxes[:, 4:7] = torch.from_numpy(half).cuda()
        balls = torch.from_numpy(pts).cuda()
        balls[:, 3] = radius

        def form(box, k, count_all, items):
            def run():
                t.set_option("closest_box", box)
                t.set_option("closest_k", k)
                t.set_option("closest_all", count_all)
                try:
                    return t.closest_points(items)
                finally:
                    t.set_option("closest_box", 0)
                    t.set_option("closest_k", 1)
                    t.set_option("closest_all", 0)
            return run
        forms = []
        for k, count_all in FORMS:
            forms.append((f"box ({k}, {count_all})", form(1, k, count_all, boxes), k))
            forms.append((f"sphere ({k}, {count_all}), R = half-diagonal", form(0, k, count_all, balls), k))
        for _, fn, _ in forms:
            fn()                                                                   # warm-up of every form
        ms = {name: [] for name, _, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn, _ in forms:
                ms[name].append(torch_time(fn))
        for name, _, _ in forms:
            rows[name] = summary(ms[name], n)
        t.set_option("closest_count", 1)
        for name, fn, k in forms:
            res = fn().reshape(n, k, 16)
            info = t.closest_info()
            counts[name] = {"node_steps_per_box": round(info["lastNodeSteps"] / n, 2), "prim_tests_per_box": round(info["lastPrimTests"] / n, 2),
                            "found": int((res[:, 0, 7].view(torch.int32) != 0).sum().item()),
                            "mean_count": round(float(res[:, 0, 14].contiguous().view(torch.int32).double().mean().item()), 3)}
        t.set_option("closest_count", 0)
        st = t.stats()

    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {G}^3 = {n} boxes, "
          f"half-extents {half.tolist()}, half-diagonal {radius:.4g}, {args.repeats} repeats")
    for name, s in rows.items():
        print(f"  {name:40s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mitems_per_s']:9.1f} M/s")
    for name, c in counts.items():
        print(f"  {name:40s} {c['node_steps_per_box']:9.2f} node steps, {c['prim_tests_per_box']:10.2f} primitive tests per box, {c['found']} found, mean count {c['mean_count']}")
    print(json.dumps({"config": args.config, "grid": G, "boxes": n, "half_extents": half.tolist(), "radius": radius, "repeats": args.repeats,
                      "rows": rows, "counts": counts}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
