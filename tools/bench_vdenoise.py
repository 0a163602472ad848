#!/usr/bin/env python3
"""Time of one rt_denoise_variance call beside one rt_denoise call (rt_vdenoise_info.lastKernelMs and rt_denoise_info.lastKernelMs: the
library's HIP events around each call's launches) on the image and the feature planes of a workload at 1080p, in one process, after a
warm-up; median [least .. largest] over the repeats.  The two filters alternate, and within each the calls with 1, 2, ... iterations
alternate in every repeat.  The parts of a call are timed by difference, as tools/bench_denoise.py does: pass i is the median of
call(i + 1) - call(i) (the last pass of a call also remodulates: one more load per pixel); call(1) of rt_denoise is the prep kernel
plus pass 0, call(1) of rt_denoise_variance is the prep kernel, the estimate pass and pass 0, so the estimate pass (with whatever pass 0
of the variance-guided filter costs more than k_atrous's: the prefilter's nine loads) is the median of their difference.

    python tools/bench_vdenoise.py --config 3
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
    ap.add_argument("--config", type=int, default=3, choices=[3, 5])
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
    ms = {name: {k: [] for k in counts} for name in ("rt_denoise", "rt_denoise_variance")}
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.render(0, args.frames)
        t.render_aov(0, args.frames)
        for rep in range(args.warmup + args.repeats):
            for k in counts:
                t.denoise(iterations=k)
                t.denoise_variance(iterations=k)
                if rep >= args.warmup:
                    ms["rt_denoise"][k].append(t.denoise_info()["lastKernelMs"])
                    ms["rt_denoise_variance"][k].append(t.vdenoise_info()["lastKernelMs"])
        st = t.stats()

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    out = {"config": args.config, "width": W, "height": H, "triangles": st["numTriangles"], "iterations": args.iterations, "repeats": args.repeats}
    for name, first in (("rt_denoise", "prep + pass 0"), ("rt_denoise_variance", "prep + estimate + pass 0")):
        m = ms[name]
        passes = []
        for i in range(args.iterations):
            s = summary(m[i + 1] if i == 0 else [a - b for a, b in zip(m[i + 1], m[i])])
            s.update(step=1 << i, what=first if i == 0 else f"pass {i}")
            passes.append(s)
        out[name] = {"call": summary(m[args.iterations]), "parts": passes}
    out["estimate_pass"] = summary([a - b for a, b in zip(ms["rt_denoise_variance"][1], ms["rt_denoise"][1])])
    out["estimate_pass"]["what"] = "call(1) of rt_denoise_variance - call(1) of rt_denoise: the estimate and the prefilter of pass 0"
    out["atrous_passes_of_the_variance_call"] = summary([a - b for a, b in zip(ms["rt_denoise_variance"][args.iterations],
                                                                               [x - y for x, y in zip(ms["rt_denoise_variance"][1], ms["rt_denoise"][1])])])
    out["atrous_passes_of_the_variance_call"]["what"] = "the call less the estimate pass: prep and the passes"
    out["call_ratio"] = round(out["rt_denoise_variance"]["call"]["median_ms"] / out["rt_denoise"]["call"]["median_ms"], 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
