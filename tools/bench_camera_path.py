#!/usr/bin/env python3
"""A moving camera accumulated frame after frame (the reference's OnRenderImage pattern: the camera is read again every frame and the
accumulation goes on), timed four ways in one process on one GPU:

  (a) per_frame    rt_set_params + rt_render_frame for every frame (one launch per frame)
  (b) queued       rt_submit_frame_params x N + rt_wait (the queue puts the run into one launch with a camera table)
  (c) batch        rt_render_params(0, N)
  (d) static       the static camera's rt_render(0, N): the roof

(a), (b) and (c) must give the same accumulation bits (asserted).  Workload: --config 3 (default) = the 100k-triangle chess scene, --config
5 = the million-triangle one with depth of field, both at 1080p, 64 rays per pixel and 8 bounces per frame; a 16-frame camera path of
small steps (as bench.py's moving-camera probe).  Writes profiles/camera_path_<config>.json.

    python tools/bench_camera_path.py [--config 3|5] [--frames 16] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_path(params, n):
    P = np.repeat(np.asarray(params).reshape(1).copy(), n)
    for f in range(n):
        d = np.float32(0.002 * (f + 1))
        P[f]["worldSpaceCameraPos"] = params["worldSpaceCameraPos"] + np.float32([d, 0.0, 0.0])
        m = P[f]["camLocalToWorld"].copy(); m[3] = params["camLocalToWorld"][3] + d; P[f]["camLocalToWorld"] = m
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=(3, 5))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = {3: rtx.scenes.config3, 5: rtx.scenes.config5}[args.config]()
    params, spheres, tris, infos = mgr.build_buffers()
    N = args.frames
    P = camera_path(params, N)
    t = rtx.Tracer(0)
    t.set_option("queue_linger_us", 100000)           # the worker waits for the N submissions (they arrive well within it) ...
    t.set_option("queue_depth", N)                    # ... and launches as soon as all N are there: one launch
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    t.reset_accum()
    t.render(0, 4)                                    # scene build, tile order, the automatic kernel choice, first use of each kernel
    t.render_params(0, P)                             # ... and of k_cam_stream

    def timed(run):
        t.reset_accum()
        t0 = time.perf_counter()
        run()
        wall = (time.perf_counter() - t0) * 1e3
        st = t.stats()
        return wall, st

    def per_frame():
        ms = 0.0
        for f in range(N):
            t.set_params(P[f]); t.render_frame(f)
            ms += t.stats()["lastKernelMs"]
        return ms

    def queued():
        for f in range(N):
            t.submit_frame_params(f, P[f])
        t.wait()

    results = {k: [] for k in ("per_frame", "queued", "batch", "static")}
    images = {}
    for rep in range(args.reps):
        for name in results:
            kern = None
            if name == "per_frame":
                t.reset_accum(); t0 = time.perf_counter(); kern = per_frame(); wall = (time.perf_counter() - t0) * 1e3; st = t.stats()
            elif name == "queued":
                wall, st = timed(queued)
            elif name == "batch":
                wall, st = timed(lambda: t.render_params(0, P))
            else:
                t.set_params(params)
                wall, st = timed(lambda: t.render(0, N))
            if kern is None:
                kern = st["lastKernelMs"]
            results[name].append({"wall_ms_per_frame": wall / N, "kernel_ms_per_frame": kern / N, "lastKernel": st["lastKernel"],
                                   "lastFramesPerLaunch": st["lastFramesPerLaunch"], "lastFramesInterleaved": st["lastFramesInterleaved"],
                                   "queuedLaunches": st["queuedLaunches"]})
            if name != "static" and rep == 0:
                images[name] = t.read_accum().view(np.uint32).copy()
    t.close()
    same = all(np.array_equal(images["per_frame"], images[k]) for k in ("queued", "batch"))
    best = {k: min(v, key=lambda r: r["wall_ms_per_frame"]) for k, v in results.items()}
    out = {
        "workload": f"config{args.config}, {int(params['width'])}x{int(params['height'])}, {int(params['numRaysPerPixel'])} rays/pixel, "
                    f"{int(params['maxBounceCount'])} bounces, {N}-frame camera path (0.002 units per frame), accumulation not reset",
        "reps": args.reps,
        "same_bits_a_b_c": bool(same),
        "best": best,
        "runs": results,
        "speedup_queued_over_per_frame": best["per_frame"]["wall_ms_per_frame"] / best["queued"]["wall_ms_per_frame"],
        "queued_share_of_static": best["static"]["wall_ms_per_frame"] / best["queued"]["wall_ms_per_frame"],
    }
    path = args.out or os.path.join(ROOT, "profiles", f"camera_path_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("workload", "same_bits_a_b_c", "speedup_queued_over_per_frame", "queued_share_of_static")}))
    for k, v in best.items():
        print(f"{k:10s} {v['wall_ms_per_frame']:8.2f} ms/frame wall, {v['kernel_ms_per_frame']:8.2f} kernel, lastKernel {v['lastKernel']}, "
              f"interleaved {v['lastFramesInterleaved']}, queued launches {v['queuedLaunches']}")
    assert same, "per-frame loop, queue and rt_render_params differ"


if __name__ == "__main__":
    main()
