#!/usr/bin/env python3
"""Paths per second of a gather query (rt_gather) beside what a caller had to do for the same estimate before it existed, in one process.

Points: the first hits of the configuration's pixel-centre camera rays (hitPoint + 1e-3 * normal, the normal; misses kept with n = 0).
`--samples` directions per point (64), both modes.  After a warm-up every form is timed `--repeats` times: median [min .. max].

  gather, host entry        rt_gather on host arrays; the time is the library's own HIP events around its launches (rt_gather_info)
  gather, device entry      rt_gather_device on a torch tensor; torch events around the call (it includes the origin-bound reduction)
  radiance n x N, device    the caller's way on the device: n * N single-sample rays (origin, a cosine-lobe direction drawn with torch —
                            the same distribution, not the library's stream) through rt_trace_radiance_device, then a torch mean over
                            each point's N results; torch events around the call and the reduction.  Making the rays is NOT timed
  radiance n x N, host      the caller's way from host memory, rt_trace_radiance with samples = 1, on a crop of the points small enough
                            to hold n * N rays in host memory; wall time of the call and a numpy mean, SCALED to all points

    python tools/bench_gather.py --config 3
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(ms, paths):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mpaths_per_s": round(paths / med * 1e-3, 1)}


def torch_timed(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 5])
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--crop", type=int, default=65536, help="points of the host-entry radiance form")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    from bench_radiance import pixel_centre_rays
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    w, h = int(params["width"]), int(params["height"])
    N = args.samples
    rows = {}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        hits = t.trace_rays(pixel_centre_rays(rtx, params))
        pts = np.zeros(len(hits), rtx.RAY)
        pts["origin"] = hits["hitPoint"] + np.float32(1e-3) * hits["normal"]
        pts["direction"], pts["tMax"] = hits["normal"], np.inf
        n = len(pts)
        paths = n * N

        dev = torch.from_numpy(pts.view(np.float32).reshape(-1, 8).copy()).cuda()    # the points on the device: (n, 8)

        # ---- the gather query
        for mode, name in ((0, "cosine"), (1, "sh9")):
            t.gather(pts, N, seed=99, mode=mode)                                     # warm-up
            ms = []
            for k in range(args.repeats):
                t.gather(pts, N, seed=k, mode=mode)
                ms.append(t.gather_info()["lastKernelMs"])
            rows[f"gather {name}, host entry (library events)"] = summary(ms, paths)
            t.gather(dev, N, seed=99, mode=mode)
            seeds = iter(range(1000))
            rows[f"gather {name}, device entry (torch events)"] = summary(torch_timed(lambda: t.gather(dev, N, seed=next(seeds), mode=mode), args.repeats), paths)

        # ---- the caller's way on the device: n x N single-sample rays, a torch reduction
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        rays = torch.zeros((n, N, 8), device="cuda")                                 # n * N * 32 B: 4.2 GB at 1080p and 64 samples
        rays[:, :, 0:3] = dev[:, None, 0:3]
        rays[:, :, 3] = float("inf")
        for k in range(N):                                                           # one sample of every point at a time: n * 12 B temporaries
            r = torch.randn((n, 3), device="cuda", generator=g)
            d = dev[:, 4:7] + r / r.norm(dim=1, keepdim=True)
            rays[:, k, 4:7] = d / d.norm(dim=1, keepdim=True)
        del r, d
        rays = rays.view(paths, 8)

        def radiance_device():
            return t.trace_radiance(rays, 1, seed=3).view(n, N, 4).mean(1)
        radiance_device()
        rows["radiance n x N, device entry + torch mean (torch events)"] = summary(torch_timed(radiance_device, args.repeats), paths)

        # ---- the caller's way from host memory, on a crop, scaled
        nc = min(args.crop, n)
        first = (n - nc) // 2
        host_rays = rays[first * N:(first + nc) * N].cpu().numpy().view(rtx.RAY).reshape(-1)
        del rays
        t.trace_radiance(host_rays[:4096], 1, seed=3)
        ms = []
        for _ in range(max(3, args.repeats // 4)):
            t0 = time.perf_counter()
            t.trace_radiance(host_rays, 1, seed=3).reshape(nc, N, 4).mean(1)
            ms.append((time.perf_counter() - t0) * 1e3 * (n / nc))
        rows[f"radiance n x N, host entry + numpy mean (wall, {nc} points SCALED to {n})"] = summary(ms, paths)
        st = t.stats()

    head = f"config {args.config}: {w} x {h}, {st['numTriangles']} triangles, {n} points ({int((hits['kind'] == 0).sum())} misses), {N} samples, {paths} paths, {args.repeats} repeats"
    print(head)
    for name, s in rows.items():
        print(f"  {name:78s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mpaths_per_s']:9.1f} Mpaths/s")
    print(json.dumps({"config": args.config, "width": w, "height": h, "points": n, "samples": N, "repeats": args.repeats, "rows": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
