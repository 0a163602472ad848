#!/usr/bin/env python3
"""Time of one radiance query (rt_trace_radiance, rt_radiance_info.lastKernelMs) of width x height pixel-centre rays at 64 samples beside
one Philox-mode image frame (rt_render_frame, rt_stats.lastKernelMs) of the same configuration, in one process: after a warm-up of both,
the two alternate and each is timed by the library's own HIP events.  Both are printed as rays of CalculateRayCollision per second.  The
frame's casts are the library's own count (rt_stats.rays).  The query has no work counters: its casts are what the DEFINITION casts
(every sample's first cast included — the kernel makes fewer, it re-enters a ray's first hit), counted on the CPU by the checker
(tests/query_oracle.c) on a sub-grid of the pixels and scaled to the image; --count-step 0 skips the count and says so.

    python tools/bench_radiance.py --config 3 --repeats 5
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pixel_centre_rays(rtx, params):
    """pinhole rays through the pixel centres, unit directions, tMax = +inf, in pixelIndex order"""
    w, h = int(params["width"]), int(params["height"])
    M = np.asarray(params["camLocalToWorld"], np.float32).reshape(4, 4)
    vp = np.asarray(params["viewParams"], np.float32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    lx, ly = ((xs + 0.5) / w - 0.5) * vp[0], ((ys + 0.5) / h - 0.5) * vp[1]
    local = np.stack([lx.ravel(), ly.ravel(), np.full(lx.size, vp[2], np.float32), np.ones(lx.size, np.float32)], 1)
    pos = np.asarray(params["worldSpaceCameraPos"], np.float32)
    d = (local @ M.T)[:, :3] - pos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(w * h, rtx.RAY)
    rays["origin"], rays["direction"], rays["tMax"] = pos, d.astype(np.float32), np.inf
    return rays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 4, 5])
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4, help="image frames before the timed ones")
    ap.add_argument("--count-step", type=int, default=24, help="the checker counts the casts of every n-th pixel in x and y (0: not counted)")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    params["rngMode"], params["numRaysPerPixel"] = 1, args.samples
    w, h = int(params["width"]), int(params["height"])
    rays = pixel_centre_rays(rtx, params)

    casts_per_ray = None
    if args.count_step > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import query_check
        sub = rays.reshape(h, w)[args.count_step // 2::args.count_step, args.count_step // 2::args.count_step].reshape(-1)
        _, casts = query_check.oracle_radiance(rtx, params, spheres, tris, infos, sub, args.samples, count_casts=True)
        casts_per_ray = casts / len(sub)

    frame_ms, query_ms = [], []
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.render(0, args.warmup)
        t.trace_radiance(rays[:w * 8], args.samples)
        rays_before = t.stats()["rays"]
        for k in range(args.repeats):
            t.render_frame(args.warmup + k)
            frame_ms.append(t.stats()["lastKernelMs"])
            t.trace_radiance(rays, args.samples, seed=k)
            query_ms.append(t.radiance_info()["lastKernelMs"])
        st, info = t.stats(), t.radiance_info()
    frame_casts = (st["rays"] - rays_before) / args.repeats

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    out = {"config": args.config, "width": w, "height": h, "samples": args.samples, "triangles": st["numTriangles"], "repeats": args.repeats,
           "philox_frame": dict(summary(frame_ms), kernel=st["lastKernel"], casts=int(frame_casts),
                                grays_per_s=round(frame_casts / statistics.median(frame_ms) * 1e-6, 3)),
           "radiance_query": dict(summary(query_ms), rays=len(rays), sample_lanes=info["lastSampleLanes"])}
    if casts_per_ray is None:
        out["radiance_query"]["casts"] = "not counted"
    else:
        casts = casts_per_ray * len(rays)
        out["radiance_query"].update(casts_of_the_definition=int(casts), counted_on_pixels=int(len(sub)),
                                     grays_per_s=round(casts / statistics.median(query_ms) * 1e-6, 3))
    out["query_over_frame_ms"] = round(statistics.median(query_ms) / statistics.median(frame_ms), 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
