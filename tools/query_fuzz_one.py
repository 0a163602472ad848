#!/usr/bin/env python3
"""One seed of tests/test_gpu_query_fuzz.py on a fresh context, with overrides of the options and of the call's settings:
tools/query_fuzz_one.py <seed> [name=value ...] (samples, first_index, seed, intersectMode or any rt_set_option name) — bisecting a
mismatch the soak run found.  Prints, per family, how many items differ from the CPU checker and the first of them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtx_pkg
import query_fuzz as qf
from query_check import oracle_hits
from ray_query_helpers import load_shim

rtx = rtx_pkg.load()
seed = int(sys.argv[1])
over = dict(a.split("=") for a in sys.argv[2:])
scene, items, options, call = qf.fuzz_case(rtx, seed, overrides=over)
p, sph, tris, infos = scene
print(f"seed {seed}: {len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres; options {options}; call {call}")


def report(what, got, want):
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
