#!/usr/bin/env python3
"""One seed of tests/test_gpu_query_fuzz.py on a fresh context, with overrides of the options and of the call's settings:
tools/query_fuzz_one.py <seed> [name=value ...] (samples, first_index, seed, intersectMode, the multi-hit form K, both_sides,
count_all, or any rt_set_option name, hits_slice and closest_slice among them) — bisecting a mismatch the soak run found.  Prints, per
family, how many items differ from the CPU checker and the first of them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtx_pkg
import closest_check as cc
import query_fuzz as qf
from query_check import oracle_hits
from ray_query_helpers import load_shim

rtx = rtx_pkg.load()
seed = int(sys.argv[1])
over = dict(a.split("=") for a in sys.argv[2:])
more, form = qf.point_knobs(seed)
form.update({k: int(over.pop(k)) for k in list(over) if k in form})
scene, items, options, call = qf.fuzz_case(rtx, seed, overrides={**more, **over})
p, sph, tris, infos = scene
points = qf.fuzz_points(rtx, seed, scene, items)
print(f"seed {seed}: {len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres; options {options}; call {call}; multi-hit form {form}")


def report(what, got, want, items=items):
    """rows of float32 words (or occlusion bytes) that differ, NaN equal to NaN"""
    g, w = np.asarray(got).reshape(len(items), -1), np.asarray(want).reshape(len(items), -1)
    same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == np.float32 else g == w
    if g.dtype == np.float32:
        same |= np.isnan(g) & np.isnan(w)
    bad = np.where(~same.all(1))[0]
    first = f", first {qf.describe(items, bad[0])}\n    got  {g[bad[0]].tolist()}\n    want {w[bad[0]].tolist()}" if len(bad) else ""
    print(f"  {what}: {len(bad)} of {len(items)} items differ{first}")


with rtx.Tracer(0) as t:
    qf.load_scene(t, scene, options)
    want = oracle_hits(rtx, load_shim(), sph, tris, infos, int(p["intersectMode"]), items)
    report("trace_rays (the 16 words as floats)", t.trace_rays(items).view(np.float32), want.view(np.float32))
    report("occluded", t.occluded(items), (want["dst"] < np.inf).astype(np.uint8))
    for family, mode in qf.FAMILIES:
        report(f"{family} mode {mode}", qf.run_family(t, items, call, family, mode), qf.checker(rtx, scene, items, call, family, mode))
    for f in (form, qf.DEEP):
        report(f"trace_hits {f} (the records' words as floats)", qf.run_hits(t, items, f).view(np.float32), qf.check_hits(rtx, scene, items, f).view(np.float32))
    report("closest_points (the 16 words as floats)", t.closest_points(points).view(np.float32),
           cc.oracle_closest(rtx, sph, tris, infos, points).view(np.float32), points)
