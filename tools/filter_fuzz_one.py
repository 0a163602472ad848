#!/usr/bin/env python3
"""One seed of tests/test_gpu_filter_fuzz.py on a fresh context: tools/filter_fuzz_one.py <seed> [name=value ...] (any rt_set_option
name) — for whoever meets a failing seed.  Prints, per plane of the seed's stages, how many pixels differ from the CPU checker, and for
the first stage that differs the first pixel and channel, with the inputs of that pixel and of its 25 pass-0 taps (the filters) or of
the pixel itself (the feature planes, the temporal step)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtx_pkg
import filter_fuzz as ff

rtx = rtx_pkg.load()
seed = int(sys.argv[1])
case = ff.fuzz_case(rtx, seed)
case["knobs"]["options"].update({k: int(v) for k, v in (a.split("=") for a in sys.argv[2:])})
p, sph, tris, infos = case["scene"]
print(f"seed {seed}: {int(p['width'])} x {int(p['height'])}, {int(p['numRaysPerPixel'])} samples, {len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres; "
      f"NaN-making elements: {case['hostile']}; knobs {case['knobs']}")
first = True
with rtx.Tracer(0) as t:
    ff.load_scene(t, case)
    for name, got, want, inputs in ff.stages(rtx, t, case):
        want = want()
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        bad = np.argwhere(~same)
        print(f"  {name}: {int((~same).any(-1).sum())} of {same.shape[0] * same.shape[1]} pixels differ")
        if len(bad) and first:
            first = False
            y, x, c = (int(v) for v in bad[0])
            print(f"    first at (x {x}, y {y}, channel {c}): got {got[y, x, c]!r} want {want[y, x, c]!r}")
            if inputs is None:
                print("    (a feature plane: its input is the scene; tests/aov_check.py oracle_frame with rect=(x, y, x + 1, y + 1) is this pixel)")
            else:
                C, A, G = inputs[:3]
                H, W = C.shape[:2]
                print(f"    the pixel: colour {C[y, x].tolist()} A {A[y, x].tolist()} G {G[y, x].tolist()}")
                if isinstance(inputs[3], dict):
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            if 0 <= y + dy < H and 0 <= x + dx < W and (dx or dy):
                                print(f"    tap ({dx:+d}, {dy:+d}): colour {C[y + dy, x + dx, :3].tolist()} A {A[y + dy, x + dx].tolist()} G {G[y + dy, x + dx].tolist()}")
                else:
                    chk = case["checker"]
                    code = chk.code[y, x]
                    print(f"    the checker's decisions: code {int(code[0]):#x} (1 valid, 2..16 tap counts, 32 history, 64 capped), x0 {int(code[1])}, y0 {int(code[2])}")
