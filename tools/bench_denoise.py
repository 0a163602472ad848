#!/usr/bin/env python3
"""Time of one rt_denoise call (rt_denoise_info.lastKernelMs: the library's HIP events around the prep kernel and the passes) on the image
and the feature planes of a workload, in one process, after a warm-up; median [least .. largest] over the repeats.  The passes are
timed by difference: calls with 1, 2, ... iterations alternate in every repeat, and pass i is the median of call(i + 1) - call(i) (the
last pass of a call also remodulates: one more load per pixel); call(1) is the prep kernel plus pass 0.  The traffic model of a pass is
25 taps x 32 B per pixel.

    python tools/bench_denoise.py --config 3 --iterations 5 --repeats 12
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
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every iteration count before the timed ones")
    ap.add_argument("--frames", type=int, default=2, help="image frames and feature frames rendered first")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    W, H = int(params["width"]), int(params["height"])
    counts = list(range(1, args.iterations + 1))
    ms = {k: [] for k in counts}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.render(0, args.frames)
        t.render_aov(0, args.frames)
        for rep in range(args.warmup + args.repeats):
            for k in counts:
                t.denoise(iterations=k)
                if rep >= args.warmup:
                    ms[k].append(t.denoise_info()["lastKernelMs"])
        st = t.stats()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    tap_bytes = 25 * 32 * W * H
    passes = []
    for i in range(args.iterations):
        d = ms[i + 1] if i == 0 else [a - b for a, b in zip(ms[i + 1], ms[i])]
        s = summary(d)
        s.update(step=1 << i, what="prep + pass 0" if i == 0 else f"pass {i}",
                 tap_GB_per_s=round(tap_bytes / (s["median_ms"] * 1e-3) / 1e9, 1) if s["median_ms"] > 0 else None)
        passes.append(s)
    print(json.dumps({"config": args.config, "width": W, "height": H, "triangles": st["numTriangles"], "iterations": args.iterations,
                      "repeats": args.repeats, "call": summary(ms[args.iterations]), "tap_bytes_per_pass": tap_bytes, "passes": passes}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
