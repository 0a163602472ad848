#!/usr/bin/env python3
"""Casts per second of a visibility gather (rt_visibility) beside the route a caller had before it existed, in one process.

Points: the first hits of the configuration's pixel-centre camera rays (hitPoint + 1e-3 * normal, the normal; misses kept with n = 0),
reach +inf.  `--samples` directions per point (64), the three modes.  After a warm-up the forms of a mode are timed alternately,
`--repeats` times each: median [min .. max].

  visibility, device entry   rt_visibility_device on a torch tensor; torch events around the call (it includes the origin-bound reduction)
  visibility, host entry     rt_visibility on host arrays; the library's own HIP events around its launches (rt_visibility_info)
  rays n x N, device         the caller's route with everything resident on the device: n * N rays (origin, a direction drawn with torch —
                             the mode's distribution, not the library's stream — reach) through rt_occluded_device (modes 0, 1) or
                             rt_trace_rays_device (mode 2), then the torch reduction to the mode's outputs; torch events around the call
                             and the reduction.  Making the rays is NOT timed
  rays n x N, host           the same route from host memory once per mode 0 / 2, rt_occluded / rt_trace_rays on a crop of the points small
                             enough to hold n * N rays in host memory; wall time of the call and a numpy mean, SCALED to all points

    python tools/bench_visibility.py --config 3
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

MODES = ((0, "cosine"), (1, "sh9"), (2, "distance"))


def summary(ms, casts):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mcasts_per_s": round(casts / med * 1e-3, 1)}


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
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--crop", type=int, default=65536, help="points of the host-memory ray route")
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
        casts = n * N
        dev = torch.from_numpy(pts.view(np.float32).reshape(-1, 8).copy()).cuda()    # the points on the device: (n, 8)
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        rays = torch.zeros((n, N, 8), device="cuda")                                 # n * N * 32 B: 4.2 GB at 1080p and 64 samples
        rays[:, :, 0:3] = dev[:, None, 0:3]
        rays[:, :, 3] = float("inf")
        nc = min(args.crop, n)
        first = (n - nc) // 2

        def draw(lobe):
            for k in range(N):                                                       # one sample of every point at a time: n * 12 B temporaries
                r = torch.randn((n, 3), device="cuda", generator=g)
                d = r / r.norm(dim=1, keepdim=True)
                if lobe:
                    d = dev[:, 4:7] + d
                    d = d / d.norm(dim=1, keepdim=True)
                rays[:, k, 4:7] = d

        for mode, name in MODES:
            draw(lobe=mode != 1)
            flat = rays.view(casts, 8)

            if mode == 0:
                def route():
                    v = 1.0 - t.occluded(flat).view(n, N).float()
                    return torch.cat([(rays[:, :, 4:7] * v[:, :, None]).mean(1), v.mean(1, keepdim=True)], 1)
            elif mode == 1:
                def route():
                    v = 1.0 - t.occluded(flat).view(n, N).float()
                    x, y, z = rays[:, :, 4], rays[:, :, 5], rays[:, :, 6]
                    Y = torch.stack([torch.full_like(x, 0.28209479), 0.48860251 * y, 0.48860251 * z, 0.48860251 * x, 1.09254843 * x * y,
                                     1.09254843 * y * z, 0.31539157 * (3.0 * z * z - 1.0), 1.09254843 * x * z, 0.54627421 * (x * x - y * y)], 2)
                    return torch.cat([(Y * v[:, :, None]).mean(1) * 12.566371, v.mean(1, keepdim=True)], 1)
            else:
                def route():
                    hit = t.trace_rays(flat).view(n, N, 16)
                    r = hit[:, :, 0]                                                 # dst: +inf for a miss, the reach here
                    return torch.stack([r.mean(1), (r * r).mean(1), torch.isfinite(r).float().mean(1)], 1)

            seeds = iter(range(1000))
            t.visibility(dev, N, seed=99, mode=mode)                                 # warm-up of every form
            route()
            a, b = [], []
            for _ in range(args.repeats):                                            # alternately: other work shares the machine
                a.append(torch_time(lambda: t.visibility(dev, N, seed=next(seeds), mode=mode)))
                b.append(torch_time(route))
            rows[f"visibility {name}, device entry (torch events)"] = summary(a, casts)
            what = "rt_trace_rays_device" if mode == 2 else "rt_occluded_device"
            rows[f"rays n x N {name}, {what} + torch reduction (torch events)"] = summary(b, casts)
            t.visibility(pts, N, seed=99, mode=mode)
            ms = []
            for k in range(args.repeats):
                t.visibility(pts, N, seed=k, mode=mode)
                ms.append(t.visibility_info()["lastKernelMs"])
            rows[f"visibility {name}, host entry (library events)"] = summary(ms, casts)
            if mode != 1:
                # the caller's route from host memory, on a crop, scaled
                host_rays = flat[first * N:(first + nc) * N].cpu().numpy().view(rtx.RAY).reshape(-1)
                call = t.trace_rays if mode == 2 else t.occluded
                call(host_rays[:4096])
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    res = call(host_rays)
                    (res["dst"] if mode == 2 else res).reshape(nc, N).mean(1)
                    ms.append((time.perf_counter() - t0) * 1e3 * (n / nc))
                what = "rt_trace_rays" if mode == 2 else "rt_occluded"
                rows[f"rays n x N {name}, {what} from host memory + numpy mean (wall, {nc} points SCALED to {n})"] = summary(ms, casts)
                del host_rays
        st = t.stats()

    head = f"config {args.config}: {w} x {h}, {st['numTriangles']} triangles, {n} points ({int((hits['kind'] == 0).sum())} misses), {N} samples, {casts} casts, {args.repeats} repeats"
    print(head)
    for name, s in rows.items():
        print(f"  {name:100s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mcasts_per_s']:9.1f} Mcasts/s")
    print(json.dumps({"config": args.config, "width": w, "height": h, "points": n, "samples": N, "repeats": args.repeats, "rows": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
