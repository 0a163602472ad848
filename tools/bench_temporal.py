#!/usr/bin/env python3
"""Time of one rt_temporal call (rt_temporal_info.lastKernelMs: the library's HIP events around the one launch) on the image and the
feature planes of a workload, in one process, after a warm-up; median [least .. largest] over the repeats.  The calls alternate between
two camera poses a small step apart, so every timed call reprojects real history (the taps are a gather).  Beside it, from the same
process, one A-trous pass of the denoiser, timed by difference as tools/bench_denoise.py does: call(2 iterations) - call(1 iteration).
The traffic model: the step reads 15 float4 per pixel (C, A, G and four taps of T', G', with N' a float each), a pass 50.

    python tools/bench_temporal.py --config 3 --repeats 12
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 4, 5])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds before the timed ones")
    ap.add_argument("--step", type=float, default=0.02, help="the camera's sideways step between the two poses, in world units")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    W, H = int(params["width"]), int(params["height"])
    moved = params.copy()
    right = np.asarray(params["camLocalToWorld"], np.float32).reshape(4, 4)[:3, 0]
    offset = (right / np.linalg.norm(right) * np.float32(args.step)).astype(np.float32)
    M = np.asarray(params["camLocalToWorld"], np.float32).reshape(4, 4).copy()
    M[:3, 3] += offset
    moved["camLocalToWorld"] = M.reshape(16)
    moved["worldSpaceCameraPos"] = np.asarray(params["worldSpaceCameraPos"], np.float32) + offset
    step_ms, one, two, with_history = [], [], [], []
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.render(0, 1)
        t.render_aov(0, 1)
        # (the image and the planes stay those of the first pose: the step's cost does not depend on what the colours are, and the
        # guides of a pose 2 cm away pass the same tests)
        for rep in range(args.warmup + args.repeats):
            for p in (moved, params):
                t.set_params(p)
                t.temporal()
                if rep >= args.warmup:
                    step_ms.append(t.temporal_info()["lastKernelMs"])
            t.denoise(iterations=1)
            a = t.denoise_info()["lastKernelMs"]
            t.denoise(iterations=2)
            b = t.denoise_info()["lastKernelMs"]
            if rep >= args.warmup:
                one.append(a)
                two.append(b)
        with_history = float((t.read_temporal_history() > 1).mean())
        st = t.stats()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    s, p = summary(step_ms), summary([b - a for a, b in zip(one, two)])
    read_bytes = (15 * 16 + 4 * 4) * W * H
    print(json.dumps({"config": args.config, "width": W, "height": H, "triangles": st["numTriangles"], "repeats": args.repeats,
                      "pixels_with_history": round(with_history, 4), "temporal": s, "atrous_pass_1": p,
                      "temporal_over_pass": round(s["median_ms"] / p["median_ms"], 3) if p["median_ms"] > 0 else None,
                      "temporal_read_GB_per_s": round(read_bytes / (s["median_ms"] * 1e-3) / 1e9, 1) if s["median_ms"] > 0 else None}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
