"""Scenes that change under one live context (tests/dynamic_fuzz.py): hostile local meshes in hostile poses, resident triangles that
deform, world-space re-uploads and a camera that leaves and returns, one after the other through the three doors of a context.  After
every step the device's world geometry is expected_world's bytes, the tree passes the audit in both node forms, the frames are the
oracle's bit for bit, the queries are a fresh context's, and the build, rebuild, repad and camera-ray-list counters move as the door says
(check_counters, lists_eligible); one test counts, over the default seeds, that every one of those paths was taken."""
import os

import numpy as np
import pytest

import dynamic_fuzz as df
from bvh_audit import aimed_rays
from device_geometry_helpers import DeviceMemory, assert_same, fresh_snapshot, query_rays, snapshot
from test_gpu_bvh_audit import audit_tracer
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu
_FIRST = int(os.environ.get("RTX_FUZZ_FIRST", "0"))
SEEDS = range(_FIRST, _FIRST + int(os.environ.get("RTX_FUZZ_SEEDS", "12")))       # RTX_FUZZ_SEEDS=100 for a soak run


def step_rays(rtx, case, s):
    """query_rays of the step's world, 64 of the rays aimed at its box faces (finite ones), and far origins on a camera step"""
    with np.errstate(all="ignore"):
        rays = [query_rays(rtx, s["params"], case[1], s["tris"])]
        aimed, _ = aimed_rays(rtx, s["tris"])
        ok = np.isfinite(aimed["origin"]).all(1) & (np.abs(aimed["origin"]) < 1e30).all(1)
    aimed = aimed[ok]
    if len(aimed):
        rays.append(aimed[np.linspace(0, len(aimed) - 1, 64).astype(int)])
    if s["step"]["door"] == "camera":
        rays.append(df.far_rays(rtx, s))
    return np.concatenate(rays)


COMPUTED = ("posA", "posB", "posC", "normalA", "normalB", "normalC", "boundsMin", "boundsMax")    # what the marshal computes; the rest it copies


def same_bytes(field, got, want):
    """byte for byte.  In the fields the marshal computes (every one is the result of rot * (s o p) + pos or of the box loop, none a
    copy of an input) a NaN equals a NaN: IEEE 754 leaves the sign and payload of an operation's NaN result to the implementation, and
    the device's differ from the host processor's (0xFFC00000 against 0x7FC00000).  Indices, counts and materials are copies: strict."""
    if field not in COMPUTED:
        return got.tobytes() == want.tobytes()
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def with_mesh(rtx, shot, chunks):
    """a world-space context's query records as the local door gives them: a triangle's `mesh` is its chunk's meshIndex (HIT, CLOSEST
    and MULTIHIT keep kind, chunk and mesh at the same offsets of their 64 bytes)"""
    out = dict(shot)
    for k in ("trace_rays", "closest_points", "trace_hits"):
        rec = np.frombuffer(shot[k], rtx._cabi.HIT).copy()
        tri = rec["kind"] == rtx._cabi.RT_HIT_TRIANGLE
        rec["mesh"][tri] = chunks["meshIndex"].astype(np.int32)[rec["chunk"][tri]]
        out[k] = rec.tobytes()
    return out


def stats_of(t):
    st = t.stats()
    return {k: st[k] for k in df.STAT_KEYS}


def crossed(st):
    """the area rule's condition as the stats show it (a NaN ratio crosses nothing)"""
    return bool(st["refitAreaRatio"] > df.REBUILD_PERCENT / 100.0)


def check_counters(s, before, mid, after, device_bvh, what):
    """bvhBuilds / bvhRebuilds over the step (before -> mid: the step and its first frames; mid -> after: the queries, whose far origins
    can make the local door refit once more, and the frames a re-upload traces afterwards).
    - a door change or a re-upload is exactly one build, and the local door and a re-upload check no area on the way in;
    - a pose, a deformation or a camera move on a standing tree builds nothing, unless the refitted tree's area crossed rebuild_percent
      of the built tree's: then exactly one build and one bvhRebuilds.  The rule is in force when the built tree has an area (> 0; NaN
      is not) and, in the local door, device_bvh is not 0; out of force nothing is rebuilt;
    - a step that rebuilt nothing keeps the node count; the world-space doors never rebuild for a camera, the local door never repads."""
    door, stands_in = s["step"]["door"], s["door"]
    builds, rebuilds = mid["bvhBuilds"] - before["bvhBuilds"], mid["bvhRebuilds"] - before["bvhRebuilds"]
    info = (what, before, mid, after)
    if door == "reupload" or (s["entered"] and door == "transforms"):
        assert (builds, rebuilds) == (1, 0), info
    elif s["entered"]:                                      # resident triangles: the build of the base, then the update by the area rule
        # (the base's built area is not in the stats any more after a rebuild; the rule is in force when it is > 0, and a tree that
        # stayed shows it: after a rebuild the ratio tells alone)
        in_force = rebuilds == 1 or mid["bvhInternalArea"] > 0
        assert builds == 1 + rebuilds and rebuilds == (1 if in_force and crossed(mid) else 0), info
    elif stands_in == "transforms" or door == "deform":     # a standing tree: refit (the camera of a local scene refits too), or the area rule
        in_force = before["bvhInternalArea"] > 0 and (stands_in != "transforms" or device_bvh != 0)
        if door == "camera" and mid["refitAreaRatio"] == before["refitAreaRatio"] and rebuilds == 0:
            in_force = False                                # (the padding already covered the camera: no pass ran)
        assert builds == rebuilds == (1 if in_force and crossed(mid) else 0), info
    else:                                                   # the camera of a world-space scene: a repad at the most
        assert (builds, rebuilds) == (0, 0), info
    if builds == 0:
        assert mid["numBvhNodes"] == before["numBvhNodes"], info
    if stands_in == "transforms":
        assert after["bvhRepads"] == before["bvhRepads"], info
    late_builds, late_rebuilds = after["bvhBuilds"] - mid["bvhBuilds"], after["bvhRebuilds"] - mid["bvhRebuilds"]
    assert late_builds == late_rebuilds and (late_rebuilds == 0 or (stands_in == "transforms" and device_bvh != 0 and crossed(after))), info


def lists_eligible(params, kernel, st):
    """rt_render.hip ensure_primary_lists: k_stream (kernel 1, or the counter-based mode under either), a fixed camera origin, a tree"""
    return (kernel == 1 or int(params["rngMode"]) == 1) and float(params["defocusStrength"]) == 0.0 and st["numBvhNodes"] > 0 and st["bvhMaxStack"] <= 160


def run_case(rtx, oracle, case, upto=None, report=None):
    """every step of the case on one context, every check after every step.  -> the counters before / after each step"""
    seed, spheres = case.seed, case[1]
    kernels = (0, 1) if seed % 4 == 0 else (case.kernel,)
    trail = []
    with rtx.Tracer(0) as t, DeviceMemory() as mem:
        for k, v in case.knobs.items():
            t.set_option(k, v)
        t.set_rows(0, int(case[0]["height"]))
        device_bvh = case.knobs["device_bvh"]
        for s in df.replay(case, upto):
            i, st = s["index"], s["step"]
            what = f"seed {seed} step {i} ({st['door']} {st['kind']})"
            before = stats_of(t) if i else dict.fromkeys(df.STAT_KEYS, 0)
            if st["door"] == "reupload":
                device_bvh = st["device_bvh"]
            df.apply_step(t, mem, case, s, frame=i)
            b = (s["params"], spheres, s["tris"], s["infos"])
            # -- frames, bit for bit the oracle's on expected_world
            mid = None
            for kernel in kernels:
                t.set_option("kernel", kernel)
                t.reset_accum()
                lists = t.stats()["primaryListBuilds"]
                t.render(i, 2)
                rays = t.stats()["rays"]
                if mid is None:
                    # every step changed the geometry or the camera, and the lists' key holds the params and scene_version: the first
                    # k_stream frames after it build the camera-ray lists anew, once, and frames of the same camera and scene after that
                    # keep them.  (Only a step whose params are the step before's shows that scene_version moved; on a camera step and
                    # the step after one the params differ anyway.)
                    mid = stats_of(t)
                    assert mid["primaryListBuilds"] - lists == (1 if lists_eligible(s["params"], kernel, mid) else 0), (what, kernel, before, mid)
                    t.render(i + 2, 1)
                    assert t.stats()["primaryListBuilds"] == mid["primaryListBuilds"], (what, kernel, "lists rebuilt for the same camera and scene")
                    t.reset_accum()
                    t.render(i, 2)
                want_acc, want_last, cnt = oracle.render(*b, i, 2, accel=True)
                assert_bitwise(t.read_last_frame(), want_last, f"{what}, kernel {kernel}, last frame")
                assert_bitwise(t.read_accum(), want_acc, f"{what}, kernel {kernel}, accum")
                assert rays == cnt["rays"], what
            # -- the world geometry the local door made
            if s["door"] == "transforms":
                dtris, dinfos = t.read_world_geometry()
                for f in dtris.dtype.names:
                    assert same_bytes(f, dtris[f], s["tris"][f]), f"{what}: triangles.{f} differ"
                for f in dinfos.dtype.names:
                    assert same_bytes(f, dinfos[f], s["infos"][f]), f"{what}: meshinfo.{f} differ: {dinfos[f]} {s['infos'][f]}"
            # -- the tree, whole
            stood = not (s["entered"] or st["door"] == "reupload") and stats_of(t)["bvhBuilds"] == before["bvhBuilds"]
            refitted = stood and (st["door"] in ("transforms", "deform") or (s["door"] != "transforms" and stats_of(t)["bvhRepads"] > before["bvhRepads"]))
            audit_tracer(t, s["tris"], f"{what}, {'refitted' if refitted else 'built or left'}", refitted=refitted)
            # -- the queries: a fresh context given expected_world from host memory
            q = step_rays(rtx, case, s)
            got = snapshot(rtx, t, s["params"], q, frames=False)
            want = fresh_snapshot(rtx, b, q, frames=False)
            if s["door"] == "transforms":
                want = with_mesh(rtx, want, case[3])
            assert_same(got, want, what)
            with np.errstate(invalid="ignore"):
                finite = np.isfinite(q["origin"]).all(1) & np.isfinite(q["direction"]).all(1)
            # -- a ray with finite numbers has a distance that is a number, and so has every surface a query names
            hits = np.frombuffer(got["trace_rays"], rtx._cabi.HIT)
            assert not np.isnan(hits["dst"][finite]).any(), what
            for name, dtype, per_ray in (("closest_points", rtx._cabi.CLOSEST, 1), ("trace_hits", rtx._cabi.MULTIHIT, 4)):
                rec = np.frombuffer(got[name], dtype)
                named = (rec["kind"] != rtx._cabi.RT_HIT_NONE) & np.repeat(finite, per_ray)
                assert not np.isnan(rec["dst"][named]).any(), f"{what}: {name} names a surface at a NaN distance"
            if i % 2 == 1:                                          # the feature planes every other step
                planes = {}
                for who, ctx in (("live", t), ("fresh", None)):
                    with (rtx.Tracer(0) if ctx is None else _keep(ctx)) as c:
                        if ctx is None:
                            c.set_option("device_bvh", 1); c.set_params(s["params"])
                            c.upload(spheres=spheres, triangles=s["tris"], meshinfo=s["infos"])
                        c.set_option("kernel", -1)
                        c.reset_aov()
                        c.render_aov(0, 2)
                        planes[who] = {f"aov {w}": c.read_aov(w).tobytes() for w in range(rtx._cabi.RT_AOV_COUNT)}
                assert_same(planes["live"], planes["fresh"], what)
            audit_tracer(t, s["tris"], f"{what}, after the queries")
            df.after_step(t, s, frame=i)
            after = stats_of(t)
            check_counters(s, before, mid, after, device_bvh, what)
            trail.append((s, before, mid, after))
            if report:
                report(what, before, after)
    return trail


class _keep:
    """`with _keep(t)`: t, left open"""
    def __init__(self, t): self.t = t
    def __enter__(self): return self.t
    def __exit__(self, *exc): return False


TRAILS = {}              # seed -> run_case's trail, for the aggregate test below


@pytest.mark.parametrize("seed", SEEDS)
def test_dynamic_scene_through_the_three_doors(rtx, oracle, seed):
    TRAILS[seed] = run_case(rtx, oracle, df.dynamic_case(rtx, seed))


def test_the_default_seeds_take_every_path(rtx, oracle):
    """counted from the stats deltas of seeds 0..11 (the trails of the test above; a seed that has not run is run here): every path
    through which a standing scene changes, and every choice of builder a re-upload can meet, occurred"""
    seen = dict.fromkeys(("refit without a rebuild", "rebuild by the area rule, local meshes", "rebuild by the area rule, resident triangles", "repad", "repad for a camera that left",
                          "deform update in place", "automatic device build of a re-uploaded scene", "return to a host build"), 0)
    for seed in range(12):
        if seed not in TRAILS:
            TRAILS[seed] = run_case(rtx, oracle, df.dynamic_case(rtx, seed))
        for s, before, mid, after in TRAILS[seed]:
            door, standing = s["step"]["door"], not s["entered"]
            builds, rebuilds = mid["bvhBuilds"] - before["bvhBuilds"], mid["bvhRebuilds"] - before["bvhRebuilds"]
            seen["refit without a rebuild"] += door == "transforms" and standing and builds == 0
            seen["rebuild by the area rule, local meshes"] += door == "transforms" and standing and (builds, rebuilds) == (1, 1)
            seen["rebuild by the area rule, resident triangles"] += door == "deform" and rebuilds == 1
            seen["repad"] += after["bvhRepads"] > before["bvhRepads"]
            seen["repad for a camera that left"] += door == "camera" and mid["bvhRepads"] > before["bvhRepads"]
            seen["deform update in place"] += door == "deform" and standing and builds == 0 and mid["numBvhNodes"] == before["numBvhNodes"]
            if door == "reupload":
                seen["automatic device build of a re-uploaded scene"] += s["step"]["device_bvh"] == -1 and mid["bvhBuiltOnDevice"] == 1
                seen["return to a host build"] += before["bvhBuiltOnDevice"] == 1 and mid["bvhBuiltOnDevice"] == 0
    print(seen)
    assert all(seen.values()), seen


def test_seed_0_through_rt_multi(rtx):
    """seed 0's steps on three contexts of device 0: frames and ray queries are the single context's, bit for bit"""
    case = df.dynamic_case(rtx, 0)
    steps = df.replay(case)
    want = []
    with rtx.Tracer(0) as t, DeviceMemory() as mem:
        t.set_option("kernel", 1)
        for s in steps:
            df.apply_step(t, mem, case, s, frame=s["index"])
            t.reset_accum()
            t.render(s["index"], 2)
            q = step_rays(rtx, case, s)
            want.append((t.read_accum().tobytes(), t.trace_rays(q).tobytes(), t.occluded(q).tobytes()))
            df.after_step(t, s, frame=s["index"])
    with DeviceMemory() as mem, rtx.MultiTracer([0, 0, 0]) as m:
        m.set_option("kernel", 1)
        for s in steps:
            df.apply_step(m, mem, case, s, frame=s["index"])
            m.reset_accum()
            m.render(s["index"], 2)
            q = step_rays(rtx, case, s)
            got = (m.read_accum().tobytes(), m.trace_rays(q).tobytes(), m.occluded(q).tobytes())
            assert got == want[s["index"]], f"step {s['index']} ({s['step']['door']} {s['step']['kind']}): {[a == b for a, b in zip(got, want[s['index']])]}"
            df.after_step(m, s, frame=s["index"])
