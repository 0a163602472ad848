"""Triangles from device memory (option "device_geometry", Tracer.upload_triangles_device): the same scene through both doors gives the
same bits; a deformation is updated in place — no build — and still gives the bits of a fresh context, with a tree that passes the audit;
the area rule rebuilds; everything that is not a deformation is a new scene; refusals change nothing; rt_multi fans a resident scene
out.  Device memory comes from the HIP runtime the library loaded (tests/device_geometry_helpers.py); the torch tensor door, on-device
displacement and stream ordering run in a process that imports torch first (tests/device_geometry_torch_worker.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from device_geometry_helpers import (COUNTS, DeviceMemory, assert_same, displaced, fresh_snapshot, query_rays, small_scene, snapshot)
from ray_query_helpers import make_rays
from test_gpu_bvh_audit import audit_tracer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def device_tracer(rtx, mem, scene, **options):
    """a context that received `scene`'s triangles from device memory (not yet built)"""
    params, spheres, tris, infos = scene
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=spheres, meshinfo=infos)
    t.upload_triangles_device(*mem.put(tris))
    return t


@pytest.mark.parametrize("n", COUNTS)
def test_same_scene_through_both_doors(rtx, n):
    """both node forms, max_leaf 1..4, both intersect modes; at 257 also 1e4 away from the origin"""
    for far in ((0.0, 1.0e4) if n == 257 else (0.0,)):
        scene = small_scene(rtx, n, far)
        rays = query_rays(rtx, *scene[:3])
        for compact, max_leaf, mode in ((1, 2, 0), (0, 1, 1), (1, 3, 1), (0, 4, 0)):
            params = scene[0].copy(); params["intersectMode"] = mode
            sc = (params,) + scene[1:]
            opts = {"compact_nodes": compact, "max_leaf": max_leaf}
            want = fresh_snapshot(rtx, sc, rays, **opts)
            with DeviceMemory() as mem, device_tracer(rtx, mem, sc, **opts) as t:
                got = snapshot(rtx, t, params, rays)
                st = t.stats()
            assert_same(got, want, f"{n} triangles, far {far}, f16 nodes {compact}, max_leaf {max_leaf}, mode {mode}")
            assert st["numTriangles"] == n and st["bvhBuiltOnDevice"] == 1 and st["bvhBuilds"] == 1


@pytest.mark.parametrize("n,far", [(1, 0.0), (2, 0.0), (5, 0.0), (64, 0.0), (65, 0.0), (257, 0.0), (257, 1.0e4)])
def test_deformation_sequence_is_updated_in_place(rtx, n, far):
    scene = small_scene(rtx, n, far)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)
    with DeviceMemory() as mem, device_tracer(rtx, mem, scene, rebuild_percent=0) as t:
        t.render(0, 1)
        st0 = t.stats()
        assert st0["bvhBuilds"] == 1 and st0["numTriangles"] == n
        for step in range(1, 7):
            now = displaced(tris, step)
            t.upload_triangles_device(*mem.put(now))
            got = snapshot(rtx, t, params, rays, frames=step in (1, 6))
            st = t.stats()
            assert (st["bvhBuilds"], st["bvhRebuilds"], st["numTriangles"], st["numBvhNodes"]) == (1, 0, n, st0["numBvhNodes"]), (step, st)
            assert st["lastGeometryMs"] > 0.0
            assert_same(got, fresh_snapshot(rtx, (params, spheres, now, infos), rays, frames=step in (1, 6)), f"{n} triangles, step {step}")
            audit_tracer(t, now, f"{n} triangles after deformation step {step}", refitted=True)


@pytest.mark.parametrize("percent,rebuilds", [(200, 1), (0, 0)])
def test_scrambled_positions_and_the_rebuild_rule(rtx, percent, rebuilds):
    scene = small_scene(rtx, 257)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)
    rng = np.random.default_rng(9)
    scrambled = tris.copy()
    shift = rng.uniform(-40, 40, (len(tris), 3)).astype(np.float32)          # every triangle goes somewhere else: the old topology is worthless
    for k in ("posA", "posB", "posC"):
        scrambled[k] = tris[k] + shift
    with DeviceMemory() as mem, device_tracer(rtx, mem, scene, rebuild_percent=percent) as t:
        t.render(0, 1)
        st0 = t.stats()
        t.upload_triangles_device(*mem.put(scrambled))
        got = snapshot(rtx, t, params, rays)
        st = t.stats()
        print(f"rebuild_percent {percent}: refitAreaRatio {st['refitAreaRatio']:.2f}")
        assert st["bvhRebuilds"] == st0["bvhRebuilds"] + rebuilds and st["bvhBuilds"] == st0["bvhBuilds"] + rebuilds, st
        assert st["refitAreaRatio"] > 2.0 or percent == 0
        audit_tracer(t, scrambled, f"scrambled, rebuild_percent {percent}", refitted=not rebuilds)
    assert_same(got, fresh_snapshot(rtx, (params, spheres, scrambled, infos), rays), f"scrambled, rebuild_percent {percent}")


@pytest.mark.parametrize("case", ["changed count", "new meshinfo", "new spheres", "host upload in between", "builder option"])
def test_what_is_not_a_deformation_is_a_new_scene(rtx, case):
    scene = small_scene(rtx, 65)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)
    now, now_infos, now_spheres = displaced(tris, 2), infos, spheres
    with DeviceMemory() as mem, device_tracer(rtx, mem, scene) as t:
        t.render(0, 1)
        builds = t.stats()["bvhBuilds"]
        opts = {}
        if case == "changed count":
            now = now[:64]                                            # (the chunk's 64 triangles: the one no chunk addressed is gone)
        elif case == "new meshinfo":
            now_infos = infos.copy(); now_infos["material"]["colour"] = (0.1, 0.9, 0.1, 1)
            t.upload(meshinfo=now_infos)
        elif case == "new spheres":
            now_spheres = spheres.copy(); now_spheres["radius"] = 0.7
            t.upload(spheres=now_spheres)
        elif case == "host upload in between":
            t.upload(triangles=tris)
            t.render(1, 1)
            assert t.stats()["bvhBuilds"] == builds + 1
            builds += 1
        else:
            t.set_option("max_leaf", 3); opts["max_leaf"] = 3
        t.upload_triangles_device(*mem.put(now))
        got = snapshot(rtx, t, params, rays)
        st = t.stats()
        assert st["bvhBuilds"] == builds + 1 and st["bvhRebuilds"] == 0 and st["numTriangles"] == len(now) and st["bvhBuiltOnDevice"] == 1, (case, st)
        audit_tracer(t, now, case)
    assert_same(got, fresh_snapshot(rtx, (params, now_spheres, now, now_infos), rays, **opts), case)


def test_far_query_origins_repad_an_updated_tree(rtx):
    scene = small_scene(rtx, 257)
    params, spheres, tris, infos = scene
    now = displaced(tris, 3)
    centre = np.float32([0.0, 1.5, 1.0])
    o = centre[None] + np.float32([[0, 1e5, 0], [1e5, 0, 0], [0, 0, -1e5], [3e4, 3e4, 3e4]])
    far = make_rays(rtx, o, centre[None] - o)
    near = query_rays(rtx, params, spheres, tris)
    # (rebuild_percent 0: padding for origins 1e5 away is 0.4 per face, which alone takes the area of boxes this small past 200 % of
    # the build's — the next update would rebuild once, as it does for local meshes, and this test is about the tree that stays)
    with DeviceMemory() as mem, device_tracer(rtx, mem, scene, rebuild_percent=0) as t:
        t.render(0, 1)
        t.upload_triangles_device(*mem.put(now))
        t.render(1, 1)                                                # the update
        st0 = t.stats()
        got_far = snapshot(rtx, t, params, far, frames=False)
        st = t.stats()
        assert st["bvhRepads"] >= st0["bvhRepads"] + 1 and st["bvhBuilds"] == st0["bvhBuilds"] == 1
        audit_tracer(t, now, "far origins over an updated tree", refitted=True)
        got_near = snapshot(rtx, t, params, near)
        t.upload_triangles_device(*mem.put(displaced(tris, 4)))       # ... and the re-padded tree takes the next update
        got_next = snapshot(rtx, t, params, near, frames=False)
        assert t.stats()["bvhBuilds"] == 1
        audit_tracer(t, displaced(tris, 4), "an update after the re-padding", refitted=True)
    assert_same(got_far, fresh_snapshot(rtx, (params, spheres, now, infos), far, frames=False), "far origins")
    assert_same(got_near, fresh_snapshot(rtx, (params, spheres, now, infos), near), "near rays after the re-padding")
    assert_same(got_next, fresh_snapshot(rtx, (params, spheres, displaced(tris, 4), infos), near, frames=False), "the update after the re-padding")


@pytest.mark.parametrize("contexts,peer", [(2, 0), (2, 1), (3, 0), (3, 1)])
def test_rt_multi_from_a_resident_source(rtx, contexts, peer):
    scene = small_scene(rtx, 257)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)
    steps = [tris, displaced(tris, 1), displaced(tris, 2)]
    want = []
    for now in steps:
        with rtx.Tracer(0) as t:
            t.set_option("device_bvh", 1); t.set_option("kernel", 1)
            t.set_params(params)
            t.upload(spheres=spheres, triangles=now, meshinfo=infos)
            t.render(0, 2)
            want.append((t.read_accum().tobytes(), t.trace_rays(rays).tobytes(), t.occluded(rays).tobytes()))
    with DeviceMemory() as mem, rtx.MultiTracer([0] * contexts) as m:
        m.set_option("peer_copies", peer); m.set_option("kernel", 1)
        m.set_params(params)
        m.upload(spheres=spheres, meshinfo=infos)
        for step, now in enumerate(steps):
            m.upload_triangles_device(*mem.put(now))
            m.reset_accum()
            m.render(0, 2)
            got = (m.read_accum().tobytes(), m.trace_rays(rays).tobytes(), m.occluded(rays).tobytes())
            assert got == want[step], f"{contexts} contexts, peer_copies {peer}, step {step}"
            assert m.info()["bvhBuilds"] == 1 and m.stats()["numTriangles"] == 257       # (one build, then updates on the first context)


def test_refusals_change_nothing(rtx):
    scene = small_scene(rtx, 65)
    params, spheres, tris, infos = scene
    rays = query_rays(rtx, params, spheres, tris)
    other = displaced(tris, 3)
    with DeviceMemory() as mem, device_tracer(rtx, mem, scene) as t:
        t.set_option("kernel", 1)
        t.render(0, 2)
        image, st0 = t.read_accum().tobytes(), t.stats()
        ptr, n = mem.put(other)
        refusals = [("a misaligned pointer", lambda: t.upload_triangles_device(ptr + 2, n - 1), "-2"),
                    ("n < 0", lambda: t.upload_triangles_device(ptr, -1), "-2")]
        for what, call, code in refusals:
            with pytest.raises(rtx.RtError, match=rf"\({code}\)"):
                call()
            st = t.stats()
            assert t.read_accum().tobytes() == image and st == st0 and st["numRenderedFrames"] == 2, what
        t.set_option("device_geometry", 0)
        with pytest.raises(rtx.RtError, match="device_geometry is 0"):    # refused in Python: the pointer never goes down as host memory
            t.upload_triangles_device(ptr, n)
        assert t.read_accum().tobytes() == image and t.stats() == st0
        t.set_option("device_geometry", 1)
        t.render(2, 1)                                                    # the scene is still the first one: no build, no update
        st = t.stats()
        assert (st["bvhBuilds"], st["numRenderedFrames"], st["lastGeometryMs"]) == (1, 3, st0["lastGeometryMs"])
        got = snapshot(rtx, t, params, rays)
    assert_same(got, fresh_snapshot(rtx, scene, rays), "after the refusals")


def test_host_uploads_do_not_see_the_option(rtx):
    scene = small_scene(rtx, 257)
    rays = query_rays(rtx, *scene[:3])
    shots = [fresh_snapshot(rtx, scene, rays, device_geometry=v, device_bvh=bvh) for bvh in (0, 1) for v in (0, 1)]
    assert_same(shots[1], shots[0], "host builder: option 1 against 0")
    assert_same(shots[3], shots[2], "device builder: option 1 against 0")


def test_torch_tensors_on_device_displacement_and_stream_order():
    """(in a fresh process that imports torch first: tests/device_geometry_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_geometry_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device geometry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
