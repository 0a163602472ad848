#!/usr/bin/env python3
"""Rays per second of sphere-cast-all (option "hits_sweep" = 1 on rt_trace_hits) beside its two baselines in one process: the sphere cast
of the same rays ("sweep" = 1 on rt_trace_rays: what K = 1 pays for the list) and rt_trace_hits at the same K (what the ball costs over
the ray).

Rays: `--width` x `--height` pixel-centre camera rays of the configuration, resident on the device; the ball's radius is 0.01 and 0.1
scene extents, as tools/bench_sweep.py has them.  Forms: K = 1, 4, 8 and K = 4 with countAll.  After a warm-up of every form the forms
are timed alternately, `--repeats` times each: median [min .. max].  All through the device entries on torch tensors, torch events around
the call (it includes the origin-bound reduction); "hits_slice" = 4194304 so that a call is one launch, as tools/bench_hits.py has it.

    python tools/bench_sweep_all.py --config 3          (writes profiles/sweep_all_timing.txt; --out elsewhere)
"""
import argparse
import json
import os
import sys

import torch  # noqa: F401  (before the library is loaded: torch brings its own HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_closest import summary, torch_time  # noqa: E402

FORMS = ((1, False), (4, False), (8, False), (4, True))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, default=3, choices=[3, 5])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_all_timing.txt"))
    args = ap.parse_args(argv)

    import rtx_pkg
    rtx = rtx_pkg.load()
    mgr = getattr(rtx.scenes, f"config{args.config}")()
    params, spheres, tris, infos = mgr.build_buffers()
    corners = np.concatenate([np.asarray(tris[k]).reshape(-1, 3) for k in ("posA", "posB", "posC")])
    extent = float(np.linalg.norm(corners.max(0) - corners.min(0))) / 2
    W, H = args.width, args.height
    M = np.asarray(params["camLocalToWorld"], np.float64).reshape(4, 4)
    vp = np.asarray(params["viewParams"], np.float64)
    px, py = np.meshgrid((np.arange(W) + 0.5) / W - 0.5, (np.arange(H) + 0.5) / H - 0.5)
    local = np.stack([px * vp[0], py * vp[1], np.full_like(px, vp[2]), np.ones_like(px)], -1).reshape(-1, 4)
    focus = (local @ M.T)[:, :3]
    pos = np.asarray(params["worldSpaceCameraPos"], np.float64)
    d = focus - pos
    n = W * H
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = pos, np.inf, d / np.linalg.norm(d, axis=1, keepdims=True)
    rows, mean_count, base = {}, {}, {}
    with rtx.Tracer(0) as t:
        t.set_option("hits_slice", 1 << 22)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        dev = torch.from_numpy(rays).cuda()
        forms = []
        for K, ca in FORMS:
            name = f"rt_trace_hits K = {K}" + (", countAll" if ca else "")
            forms.append((name, lambda K=K, ca=ca: t.trace_hits(dev, K, False, ca)))
            base[K, ca] = name
        for frac in (0.01, 0.1):
            r = frac * extent
            forms.append((f"sphere_cast, r = {frac}", lambda r=r: rtx.sweep.sphere_cast(t, dev, r)))
            for K, ca in FORMS:
                forms.append((f"sphere_cast_all K = {K}" + (", countAll" if ca else "") + f", r = {frac}",
                              lambda r=r, K=K, ca=ca: rtx.sweep.sphere_cast_all(t, dev, r, K, ca)))
        for name, fn in forms:
            res = fn()                                                             # warm-up of every form
            if res.dim() == 3:                                                     # MULTIHIT records: word 14 is hitCount
                mean_count[name] = float(res[:, 0, 14].view(torch.int32).float().mean().item())
        ms = {name: [] for name, _ in forms}
        for _ in range(args.repeats):                                              # alternately: other work shares the machine
            for name, fn in forms:
                ms[name].append(torch_time(fn))
        for name, _ in forms:
            rows[name] = summary(ms[name], n)
        st = t.stats()
    lines = [f"config {args.config}: {st['numTriangles']} triangles, {st['numSpheres']} spheres, {st['numBvhNodes']} BVH nodes, {W} x {H} = {n} rays, "
             f"extent {extent:.4g}, median of {args.repeats} alternating repeats [min .. max]"]
    for name, s in rows.items():
        extra = f"  mean hitCount {mean_count[name]:.2f}" if name in mean_count else ""
        lines.append(f"  {name:44s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]  {s['mitems_per_s']:9.1f} Mrays/s{extra}")
    lines.append("ratios of medians:")
    for frac in (0.01, 0.1):
        cast = rows[f"sphere_cast, r = {frac}"]["median_ms"]
        for K, ca in FORMS:
            name = f"sphere_cast_all K = {K}" + (", countAll" if ca else "") + f", r = {frac}"
            lines.append(f"  {name:44s} {rows[name]['median_ms'] / cast:6.2f} x sphere_cast   {rows[name]['median_ms'] / rows[base[K, ca]]['median_ms']:6.2f} x rt_trace_hits at the same K")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"config": args.config, "rays": n, "extent": extent, "repeats": args.repeats, "rows": rows, "mean_hit_count": mean_count}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
