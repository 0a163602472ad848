#!/usr/bin/env python3
"""Rays per second of a sphere cast (option "sweep" = 1 on rt_trace_rays / rt_occluded) beside the plain ray queries of the same rays,
in one process.

Rays: `--width` x `--height` pixel-centre camera rays of the configuration, resident on the device; the ball's radius is `--radius`
scene extents (default 0.01 and 0.1 are both timed).  After a warm-up the forms are timed alternately, `--repeats` times each: median
[min .. max].  All through the device entries on torch tensors, torch events around the call (it includes the origin-bound reduction).

    python tools/bench_sweep.py --config 3 | tee profiles/sweep_timing.txt
"""
import argparse
import json
import os
import sys

import torch  # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_closest import summary, torch_time  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 5])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    corners = np.concatenate([np.asarray(tris[k]).reshape(-1, 3) for k in ("posA", "posB", "posC")])
    extent = float(np.linalg.norm(corners.max(0) - corners.min(0))) / 2
    W, H = args.width, args.height
    M = np.asarray(params["camLocalToWorld"], np.float64).reshape(4, 4)
    vp = np.asarray(params["viewParams"], np.float64)
    px, py = np.meshgrid((np.arange(W) + 0.5) / W - 0.5, (np.arange(H) + 0.5) / H - 0.5)
    local = np.stack([px * vp[0], py * vp[1], np.full_like(px, vp[2]), np.ones_like(px)], -1).reshape(-1, 4)
    focus = (local @ M.T)[:, :3]
    pos = np.asarray(params["worldSpaceCameraPos"], np.float64)
    d = focus - pos
    n = W * H
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = pos, np.inf, d / np.linalg.norm(d, axis=1, keepdims=True)
    rows, found = {}, {}
    with rtx.Tracer(0) as t:
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        dev = torch.from_numpy(rays).cuda()
        forms = [("rays, rt_trace_rays", lambda: t.trace_rays(dev)), ("rays, rt_occluded", lambda: t.occluded(dev))]
        for frac in (0.01, 0.1):
            r = frac * extent
            forms.append((f"sphere_cast, r = {frac} extents", lambda r=r: rtx.sweep.sphere_cast(t, dev, r)))
            forms.append((f"sphere_check, r = {frac} extents", lambda r=r: rtx.sweep.sphere_check(t, dev, r)))
        for name, fn in forms:
            res = fn()                                                             # warm-up of every form
            found[name] = int((res[:, 7].view(torch.int32) != 0).sum().item()) if res.dim() == 2 else int(res.sum().item())
        ms = {name: [] for name, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn in forms:
                ms[name].append(torch_time(fn))
        for name, _ in forms:
            rows[name] = summary(ms[name], n)
        st = t.stats()
    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {W} x {H} = {n} rays, extent {extent:.4g}, {args.repeats} repeats")
    for name, s in rows.items():
        print(f"  {name:40s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mitems_per_s']:9.1f} M/s  {found[name]} of {n} hit")
    print(json.dumps({"config": args.config, "rays": n, "extent": extent, "repeats": args.repeats, "rows": rows, "found": found}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
