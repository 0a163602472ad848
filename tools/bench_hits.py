#!/usr/bin/env python3
"""Rays per second of a multi-hit ray query (rt_trace_hits) beside a closest-hit ray query of the same rays, in one process.

Rays: the width x height pixel-centre camera rays of the configuration (1080p: 2.07 M), resident on the device.  After a warm-up the
forms are timed alternately, `--repeats` times each: median [min .. max].  All through the device entries on torch tensors, torch
events around the call (it includes the origin-bound reduction and its synchronisation).

  rays, rt_trace_rays        the yardstick: closest hit
  hits, K = 1 front          the same question through the list machinery: the ratio to the yardstick is its cost
  hits, K = 4 / K = 8 front  more records: more stores, a weaker pruning bound
  hits, K = 4 both sides     back faces and sphere exits as well
  hits, K = 4 countAll       no pruning by the K-th distance: every surface along the ray is visited

    python tools/bench_hits.py --config 3
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_radiance import pixel_centre_rays  # noqa: E402


def summary(ms, items):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mrays_per_s": round(items / med * 1e-3, 1)}


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
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    rays = pixel_centre_rays(rtx, params)
    n = len(rays)
    rows, counts = {}, {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.set_option("hits_slice", 1 << 22)                                        # one launch per call, as the yardstick has
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        forms = (("rays, rt_trace_rays", lambda: t.trace_rays(dev)),
                 ("hits, K = 1 front", lambda: t.trace_hits(dev, 1)),
                 ("hits, K = 4 front", lambda: t.trace_hits(dev, 4)),
                 ("hits, K = 8 front", lambda: t.trace_hits(dev, 8)),
                 ("hits, K = 4 both sides", lambda: t.trace_hits(dev, 4, True)),
                 ("hits, K = 4 front countAll", lambda: t.trace_hits(dev, 4, False, True)),
                 ("hits, K = 4 both sides countAll", lambda: t.trace_hits(dev, 4, True, True)))
        for name, fn in forms:
            res = fn()                                                             # warm-up of every form, and what it found
            if name.startswith("hits"):
                rec = res[:, 0, :].view(torch.int32)
                counts[name] = {"rays_with_a_hit": int((rec[:, 14] > 0).sum().item()), "mean_hitCount": round(float(rec[:, 14].float().mean().item()), 3)}
            else:
                counts[name] = {"rays_with_a_hit": int((res.view(torch.int32)[:, 7] != 0).sum().item())}
        ms = {name: [] for name, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn in forms:
                ms[name].append(torch_time(fn))
        for name, _ in forms:
            rows[name] = summary(ms[name], n)
        st = t.stats()

    print(f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {n} rays, {args.repeats} repeats")
    base = rows["rays, rt_trace_rays"]["median_ms"]
    for name, s in rows.items():
        c = counts[name]
        extra = f"  mean hitCount {c['mean_hitCount']}" if "mean_hitCount" in c else ""
        print(f"  {name:34s} {s['median_ms']:9.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mrays_per_s']:9.1f} Mrays/s  x{s['median_ms'] / base:5.2f}"
              f"  {c['rays_with_a_hit']} rays hit{extra}")
    print(json.dumps({"config": args.config, "rays": n, "repeats": args.repeats, "rows": rows, "counts": counts}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
