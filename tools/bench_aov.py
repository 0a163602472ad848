#!/usr/bin/env python3
"""Time of one feature frame (rt_render_aov, rt_aov_info.lastKernelMs) beside one image frame (rt_render_frame, rt_stats.lastKernelMs) of
the same workload, in one process: after a warm-up of both, single frames of the two alternate and each is timed by the library's own
HIP events.  Prints the median, the least and the largest of each.

    python tools/bench_aov.py --config 3 --repeats 12
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 4, 5])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6, help="image frames before the timed ones (the automatic kernel choice settles in the first few)")
    ap.add_argument("--rng", choices=["pcg", "philox"], default="pcg")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    params["rngMode"] = 1 if args.rng == "philox" else 0
    image_ms, feature_ms = [], []
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.render(0, args.warmup)
        t.render_aov(0, 2)
        for k in range(args.repeats):
            t.render_frame(args.warmup + k)
            image_ms.append(t.stats()["lastKernelMs"])
            t.render_aov(2 + k, 1)
            feature_ms.append(t.aov_info()["lastKernelMs"])
        st, info = t.stats(), t.aov_info()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    print(json.dumps({"config": args.config, "width": int(params["width"]), "height": int(params["height"]),
                      "rays_per_pixel": int(params["numRaysPerPixel"]), "triangles": st["numTriangles"], "rng": args.rng, "repeats": args.repeats,
                      "image_frame": dict(summary(image_ms), kernel=st["lastKernel"], rays=st["rays"]),
                      "feature_frame": dict(summary(feature_ms), sample_lanes=info["lastSampleLanes"]),
                      "feature_over_image": round(statistics.median(feature_ms) / statistics.median(image_ms), 4)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
