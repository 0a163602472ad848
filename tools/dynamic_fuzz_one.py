#!/usr/bin/env python3
"""One seed of tests/test_gpu_dynamic_fuzz.py on a fresh context: tools/dynamic_fuzz_one.py <seed> [upto=K] [door=transforms|deform|
reupload] [name=value ...] (any rt_set_option name overrides the seed's knob) — bisecting a mismatch the soak run found.  Steps 0..K
run one after the other (door=...: only the checks of steps that stand in that door are printed); per step it prints the counters, the
first output and word that differ from the oracle / a fresh context / expected_world, and the audit's report."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtx_pkg
import dynamic_fuzz as df
import oracle_binding
from bvh_audit import audit
from device_geometry_helpers import DeviceMemory, fresh_snapshot, snapshot
from test_gpu_dynamic_fuzz import stats_of, step_rays, with_mesh

rtx = rtx_pkg.load()
oracle = oracle_binding.Oracle()
seed = int(sys.argv[1])
over = dict(a.split("=") for a in sys.argv[2:])
upto = int(over.pop("upto")) if "upto" in over else None
door = over.pop("door", None)
case = df.dynamic_case(rtx, seed)
case.knobs.update({k: int(v) for k, v in over.items()})
params, spheres, local, chunks, n_meshes, steps = case
print(f"seed {seed}: {len(local)} triangles in {len(chunks)} chunks of {n_meshes} meshes, {len(spheres)} spheres, {int(params['width'])}x{int(params['height'])}, "
      f"kernel {case.kernel}; knobs {case.knobs}")


def first_word(what, got, want):
    """the first 32-bit word that differs (NaN equal to NaN where the words are floats)"""
    got, want = got + bytes(-len(got) % 4), want + bytes(-len(want) % 4)          # (occlusion answers are bytes)
    g, w = np.frombuffer(got, np.uint32), np.frombuffer(want, np.uint32)
    same = (g == w) | (np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32)))
    if len(g) != len(w) or not same.all():
        i = int(np.argmin(same)) if len(g) == len(w) else -1
        print(f"    {what}: {int((~same).sum()) if i >= 0 else 'length'} words differ; first word {i}: got {g[i]:#010x} ({g.view(np.float32)[i]}), "
              f"want {w[i]:#010x} ({w.view(np.float32)[i]})")
        return False
    return True


with rtx.Tracer(0) as t, DeviceMemory() as mem:
    for k, v in case.knobs.items():
        t.set_option(k, v)
    t.set_rows(0, int(params["height"]))
    for s in df.replay(case, upto):
        i, st = s["index"], s["step"]
        df.apply_step(t, mem, case, s, frame=i)
        t.set_option("kernel", case.kernel)
        t.reset_accum()
        t.render(i, 2)
        show = door is None or s["door"] == door
        if show:
            print(f"step {i}: {st['door']} {st['kind']} (the scene stands in {s['door']}{', entered' if s['entered'] else ''}); {stats_of(t)}")
            b = (s["params"], spheres, s["tris"], s["infos"])
            want_acc, _, cnt = oracle.render(*b, i, 2, accel=True)
            ok = first_word("frames against the oracle", t.read_accum().tobytes(), want_acc.tobytes())
            if t.stats()["rays"] != cnt["rays"]:
                print(f"    rays: {t.stats()['rays']}, the oracle's {cnt['rays']}"); ok = False
            if s["door"] == "transforms":
                dtris, dinfos = t.read_world_geometry()
                for f in dtris.dtype.names:
                    ok &= first_word(f"triangles.{f} against expected_world", dtris[f].tobytes(), s["tris"][f].tobytes())
                for f in ("boundsMin", "boundsMax"):
                    ok &= first_word(f"meshinfo.{f} against expected_world", dinfos[f].tobytes(), s["infos"][f].tobytes())
            q = step_rays(rtx, case, s)
            got, want = snapshot(rtx, t, s["params"], q, frames=False), fresh_snapshot(rtx, b, q, frames=False)
            if s["door"] == "transforms":
                want = with_mesh(rtx, want, chunks)
            for k in got:
                ok &= got[k] == want[k] or first_word(f"{k} against a fresh context", got[k], want[k])
            f32, f16 = t.read_bvh()
            sts = t.stats()
            rep = audit(f32, f16, t.read_bvh_order(), s["tris"], max_stack=sts["bvhMaxStack"], exact_stack=bool(sts["bvhBuiltOnDevice"]))
            print(f"    {'everything agrees' if ok else 'DIFFERENCES above'}; audit: {'clean, ' if rep.clean else 'FAILED '}{rep}")
        df.after_step(t, s, frame=i)
