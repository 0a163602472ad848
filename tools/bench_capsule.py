#!/usr/bin/env python3
"""Capsules per second of the capsule overlap queries (rt_closest_points with the option "closest_capsule") beside the two things a
caller without them can do at the same points, in one process.

Capsules: bench_closest.py's `--grid`^3 grid (128: 2.1 M points) over the configuration's bounding box, each point the centre of a
VERTICAL capsule (axis along y) of half-length one cell (the cell's y extent) and radius the cell's half-diagonal.  The yardsticks:

  ball       one K-nearest call at the centre with R = radius + half-length: the ball around the capsule (over-reports)
  3 balls    three K-nearest calls with R = radius at P0, the centre and P1: a string of balls along the axis (under-reports between them)

After a warm-up the forms are timed alternately, `--repeats` times each: median [min .. max].  All through the device entry on torch
tensors, torch events around the call or the three calls (they include the origin-bound reductions).  (K, all) = (1, 0) CheckCapsule,
(4, 0) the nearest four surfaces, (1, 1) the overlap count.

One more call of each capsule and ball form runs the counting kernel (option "closest_count") for the node steps and primitive tests per
query — and the same for the same capsules turned along (1, 1, 1), same length and radius: the node step's bound is the segment's
axis-aligned bounds, exact for the vertical capsule and loose for the diagonal one.  The diagonal capsules are timed too.

    python tools/bench_capsule.py --config 3
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

FORMS = ((1, 0), (4, 0), (1, 1))


def summary(ms, items):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "items": items,
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
    radius = float(np.linalg.norm(cell * np.float32(0.5)))
    half_len = float(cell[1])
    n = G ** 3
    centre = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)

    def segments(direction):
        u = np.asarray(direction, np.float32) / np.float32(np.linalg.norm(direction))
        seg = np.zeros((n, 8), np.float32)
        seg[:, 0:3] = centre - u * np.float32(half_len)
        seg[:, 3] = radius
        seg[:, 4:7] = u * np.float32(2 * half_len)
        return seg

    def points(xyz, R):
        p = np.zeros((n, 8), np.float32)
        p[:, 0:3] = xyz
        p[:, 3] = R
        return p
    rows, counts = {}, {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        vertical_np = segments((0, 1, 0))
        vertical = torch.from_numpy(vertical_np).cuda()
        diagonal = torch.from_numpy(segments((1, 1, 1))).cuda()
        ball = torch.from_numpy(points(centre, radius + half_len)).cuda()
        three = [torch.from_numpy(points(x, radius)).cuda() for x in (vertical_np[:, 0:3], centre, vertical_np[:, 0:3] + vertical_np[:, 4:7])]

        def form(capsule, k, count_all, batches):
            def run():
                t.set_option("closest_capsule", capsule)
                t.set_option("closest_k", k)
                t.set_option("closest_all", count_all)
                try:
                    return [t.closest_points(b) for b in batches]
                finally:
                    t.set_option("closest_capsule", 0)
                    t.set_option("closest_k", 1)
                    t.set_option("closest_all", 0)
            return run
        forms = []
        for k, count_all in FORMS:
            forms.append((f"capsule, vertical ({k}, {count_all})", form(1, k, count_all, [vertical]), k))
            forms.append((f"capsule, diagonal ({k}, {count_all})", form(1, k, count_all, [diagonal]), k))
            forms.append((f"ball, R + half-length ({k}, {count_all})", form(0, k, count_all, [ball]), k))
            forms.append((f"3 balls along the axis ({k}, {count_all})", form(0, k, count_all, three), k))
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
            if name.startswith("3 balls"):
                continue                            # (the counters hold one call: three calls are three times the ball's kind of walk)
            res = fn()[0].reshape(n, k, 16)
            info = t.closest_info()
            counts[name] = {"node_steps": round(info["lastNodeSteps"] / n, 2), "prim_tests": round(info["lastPrimTests"] / n, 2),
                            "found": int((res[:, 0, 7].view(torch.int32) != 0).sum().item()),
                            "mean_count": round(float(res[:, 0, 14].contiguous().view(torch.int32).double().mean().item()), 3)}
        t.set_option("closest_count", 0)
        st = t.stats()

    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {G}^3 = {n} capsules, "
          f"half-length {half_len:.4g}, radius {radius:.4g}, {args.repeats} repeats")
    for name, s in rows.items():
        print(f"  {name:40s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mitems_per_s']:9.1f} M/s")
    for k, count_all in FORMS:
        c = rows[f"capsule, vertical ({k}, {count_all})"]["median_ms"]
        print(f"  ({k}, {count_all}): vertical capsule / ball = {c / rows[f'ball, R + half-length ({k}, {count_all})']['median_ms']:.2f}, "
              f"/ 3 balls = {c / rows[f'3 balls along the axis ({k}, {count_all})']['median_ms']:.2f}, "
              f"diagonal / vertical = {rows[f'capsule, diagonal ({k}, {count_all})']['median_ms'] / c:.2f}")
    for name, c in counts.items():
        print(f"  {name:40s} {c['node_steps']:9.2f} node steps, {c['prim_tests']:10.2f} primitive tests per query, {c['found']} found, mean count {c['mean_count']}")
    print(json.dumps({"config": args.config, "grid": G, "capsules": n, "half_length": half_len, "radius": radius, "repeats": args.repeats,
                      "rows": rows, "counts": counts}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
