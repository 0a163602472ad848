#!/usr/bin/env python3
"""Ray-query throughput (rt_trace_rays / rt_occluded) on the benchmark scenes, in one process on one GPU.

Ray sets, 2,073,600 rays each (one per pixel of 1920x1080):
  camera   pinhole camera rays through the pixel centres (coherent)
  bounce   from the camera rays' hit points in uniformly random directions (incoherent)
  shadow   from the same hit points towards worldSpaceLightPos0 (occlusion queries)

Every set is timed through the host entries (numpy arrays: host -> device copies, the query, device -> host copies; wall clock), and
through the device entries on torch tensors (HIP events around the call alone: warm-up, then --reps repetitions; min / median / max),
closest hit and occlusion.  For context, the renderer's own rate on the same scene (rt_render over --frames frames: CalculateRayCollision
calls per kernel second).  --config 3 = the 100k-triangle chess scene, 5 = the million-triangle one.  Writes
profiles/ray_query_<config>.json.

    python tools/bench_ray_query.py [--config 3|5] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(rtx, params, w, h):
    M = np.asarray(params["camLocalToWorld"], np.float32).reshape(4, 4)
    vp = np.asarray(params["viewParams"], np.float32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    lx, ly = ((xs + 0.5) / w - 0.5) * vp[0], ((ys + 0.5) / h - 0.5) * vp[1]
    local = np.stack([lx.ravel(), ly.ravel(), np.full(lx.size, vp[2], np.float32), np.ones(lx.size, np.float32)], 1)
    d = (local @ M.T)[:, :3] - np.asarray(params["worldSpaceCameraPos"], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(w * h, rtx.RAY)
    r["origin"], r["direction"], r["tMax"] = params["worldSpaceCameraPos"], d, np.inf
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=(3, 5))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = {3: rtx.scenes.config3, 5: rtx.scenes.config5}[args.config](1920, 1080)
    params, spheres, tris, infos = mgr.build_buffers()
    t = rtx.Tracer(0)
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)

    cam = camera_rays(rtx, params, 1920, 1080)
    first = t.trace_rays(cam)                             # (also builds the scene)
    hit = first["kind"] != 0
    rng = np.random.default_rng(1)
    d = rng.standard_normal((len(cam), 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origins = np.where(hit[:, None], first["hitPoint"], cam["origin"])
    bounce = np.zeros(len(cam), rtx.RAY)
    bounce["origin"], bounce["direction"], bounce["tMax"] = origins, d, np.inf
    shadow = np.zeros(len(cam), rtx.RAY)
    shadow["origin"], shadow["direction"], shadow["tMax"] = origins, params["worldSpaceLightPos0"], np.inf
    sets = {"camera": cam, "bounce": bounce, "shadow": shadow}

    def host_rate(fn, rays):
        fn(rays)
        walls = []
        for _ in range(max(3, args.reps // 4)):
            t0 = time.perf_counter(); fn(rays); walls.append(time.perf_counter() - t0)
        return len(rays) / min(walls) / 1e6, [w * 1e3 for w in walls]

    side = torch.cuda.Stream()                            # (a stream with a handle: the device entries run on it, asynchronously)

    def device_rate(fn, dev):
        side.wait_stream(torch.cuda.current_stream())
        ms = []
        with torch.cuda.stream(side):
            for _ in range(args.warmup):
                fn(dev)
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side); fn(dev); e1.record(side); e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        n = dev.shape[0]
        return {"mrays_per_s_best": n / ms.min() / 1e3, "mrays_per_s_median": n / np.median(ms) / 1e3, "mrays_per_s_worst": n / ms.max() / 1e3,
                "ms_min": float(ms.min()), "ms_median": float(np.median(ms)), "ms_max": float(ms.max())}

    results = {}
    for name, rays in sets.items():
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        row = {"rays": int(len(rays))}
        for q, fn in (("closest", t.trace_rays), ("occluded", t.occluded)):
            rate, walls = host_rate(fn, rays)
            row[q] = {"host_mrays_per_s_best": rate, "host_wall_ms": walls, "device": device_rate(fn, dev)}
        row["hit_fraction"] = float((t.trace_rays(rays)["kind"] != 0).mean())
        results[name] = row
        del dev

    t.render(0, 1)                                        # scene, kernel choice, tile order
    t.render(0, args.frames)
    st = t.stats()
    render_rate = st["rays"] / st["lastKernelMs"] / 1e3
    t.close()
    out = {
        "workload": f"config{args.config}: {int(st['numTriangles'])} triangles, {int(st['numSpheres'])} spheres; 1920x1080 = {len(cam)} rays per set",
        "measured": "host entries: wall clock incl. copies (best of the repetitions); device entries: HIP events around the call on torch tensors "
                    f"({args.warmup} warm-up, {args.reps} repetitions); renderer: rt_render over {args.frames} frames, rays / kernel time",
        "not_measured": "rt_multi queries across several GPUs; batches other than 2,073,600 rays; ray reordering",
        "sets": results,
        "renderer_mrays_per_s": render_rate,
        "renderer_rays": int(st["rays"]), "renderer_kernel_ms": st["lastKernelMs"],
    }
    path = args.out or os.path.join(ROOT, "profiles", f"ray_query_{args.config}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(out["workload"])
    for name, row in results.items():
        for q in ("closest", "occluded"):
            dv = row[q]["device"]
            print(f"{name:7s} {q:8s} host {row[q]['host_mrays_per_s_best']:8.1f} Mrays/s   device {dv['mrays_per_s_median']:8.1f} Mrays/s "
                  f"(best {dv['mrays_per_s_best']:.1f}, worst {dv['mrays_per_s_worst']:.1f})   hits {row['hit_fraction']:.3f}")
    print(f"renderer {render_rate:.1f} Mrays/s")


if __name__ == "__main__":
    main()
