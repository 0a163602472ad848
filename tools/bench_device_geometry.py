#!/usr/bin/env python3
"""Per-step time of a mesh that deforms on the device, three ways (option "device_geometry", DESIGN.md "Device-resident triangles"):

  (a) update   Tracer.upload_triangles_device + the in-place update (k_deform_update, refit) + one frame
  (b) rebuild  the same upload with the update ruled out — the count alternates between n and n + 1 (one more triangle in no chunk), so
               every step is a new scene: a full device build + one frame
  (c) host     the way without the option: the tensor copied to the host, Tracer.upload from host memory, one frame (device_bvh -1: a
               scene re-sent within 16 frames goes to the device builder)

A step displaces every corner by a smooth field, computed by torch on the device.  Wall times are taken around the step with the device
synchronised at both ends, after `--warmup` untimed steps; median [least .. largest] over `--steps`.  update_ms is rt_stats.lastGeometryMs:
HIP events around the whole update (the record kernel, the 4-byte read-back, one refit launch per level, the f16 nodes, the area sum).
The traffic model of k_deform_update is 84 B in + 96 B out per triangle; update_GBps = that over update_ms, so it is a LOWER bound of the
kernel's own rate (the refit's launches are inside the time and outside the bytes).

    python tools/bench_device_geometry.py --config 3 --steps 16
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # (before the library: both then use torch's HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_TRIANGLE = 84 + 96
HBM_ATTAINABLE_GBPS = 6300          # a float4 copy's measured rate on the MI355X (8 TB/s peak)


def displace(x, step):
    p = x[:, :9].reshape(-1, 3, 3)
    d = torch.stack([torch.sin(p[..., 1] * 1.3 + step), torch.cos(p[..., 0] * 0.7 + 0.5 * step), torch.sin(p[..., 2] + p[..., 0] + step)], -1)
    out = x.clone()
    out[:, :9] = (p + 0.002 * d).reshape(-1, 9)
    return out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def run(rtx, config, steps, warmup, width, height):
    mgr = getattr(rtx.scenes, f"config{config}")(width, height)
    params, spheres, tris, infos = mgr.build_buffers()
    infos = infos.copy(); infos["boundsMin"], infos["boundsMax"] = -1.0e6, 1.0e6        # (the chunk boxes do not follow the field)
    n = len(tris)
    base = torch.from_numpy(np.ascontiguousarray(tris).view(np.float32).reshape(-1, 18).copy()).cuda()
    padded = torch.cat([base, base[-1:]])                                               # n + 1 rows: the last in no chunk
    out = {"config": config, "width": int(params["width"]), "height": int(params["height"]), "triangles": n, "steps": steps, "warmup": warmup}

    def timed(step_fn):
        wall = []
        for s in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = step_fn(s)
            torch.cuda.synchronize()
            if s >= warmup:
                wall.append(((time.perf_counter() - t0) * 1e3, extra))
        return wall

    for way in ("update", "rebuild", "host"):
        with rtx.Tracer(0) as t:
            t.set_params(params)
            t.upload(spheres=spheres, meshinfo=infos)
            if way == "host":
                t.upload(triangles=tris)
            else:
                t.upload_triangles_device(base)
            t.render(0, 1)
            state = {"x": base}

            def step(s, t=t, way=way, state=state):
                if way == "rebuild":
                    rows = n + (s & 1)
                    x = displace(padded, s)[:rows].contiguous()
                else:
                    x = displace(state["x"], s)
                    state["x"] = x
                if way == "host":
                    t.upload(triangles=x.cpu().numpy().reshape(-1).view(rtx.TRIANGLE))
                else:
                    t.upload_triangles_device(x)
                t.render_frame(1 + s)
                st = t.stats()
                return st["lastGeometryMs"], st["lastBvhBuildMs"], st["lastKernelMs"], st["bvhBuilds"], st["bvhRebuilds"]

            w = timed(step)
            st = t.stats()
        rec = {"step": summary([a for a, _ in w]), "frame_kernel": summary([e[2] for _, e in w]), "bvhBuilds": st["bvhBuilds"], "bvhRebuilds": st["bvhRebuilds"]}
        if way == "update":
            upd = summary([e[0] for _, e in w])
            rec["update_ms"] = upd
            rec["update_GBps_lower_bound"] = round(n * BYTES_PER_TRIANGLE / (upd["median_ms"] * 1e-3) / 1e9, 1)
            rec["hbm_attainable_GBps"] = HBM_ATTAINABLE_GBPS
        else:
            rec["build_ms"] = summary([e[1] for _, e in w])
        out[way] = rec
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, action="append", choices=[3, 5], help="workload(s); default 3 and 5")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/device_geometry_timing.txt)")
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    lines = ["# tools/bench_device_geometry.py: per-step time of a mesh deforming on the device, three ways (see the tool's docstring)",
             f"# {args.steps} timed steps after {args.warmup} warm-up steps, {args.width}x{args.height}, one frame per step; median [min .. max] in ms",
             "# config triangles | (a) update: step, of which update | (b) rebuild: step, of which build | (c) host: step, of which build | update GB/s (lower bound) / attainable"]
    for config in args.config or [3, 5]:
        r = run(rtx, config, args.steps, args.warmup, args.width, args.height)
        print(json.dumps(r))

        def f(s):
            return f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"
        lines.append(f"{config} {r['triangles']} | {f(r['update']['step'])}, {f(r['update']['update_ms'])} | {f(r['rebuild']['step'])}, {f(r['rebuild']['build_ms'])} | "
                     f"{f(r['host']['step'])}, {f(r['host']['build_ms'])} | {r['update']['update_GBps_lower_bound']} / {HBM_ATTAINABLE_GBPS}")
        lines.append(f"#   builds + rebuilds over the run: update {r['update']['bvhBuilds']} + {r['update']['bvhRebuilds']}, rebuild {r['rebuild']['bvhBuilds']}, host {r['host']['bvhBuilds']}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
