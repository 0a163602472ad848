"""k_stream's traversal stack around the end of its LDS part, and the per-lane fields that share a register.

The wave keeps a scalar bound on the depth of its deepest lane and takes the plain pushes and pops while that bound is inside the LDS
part; the checked, spilling forms run only once a ballot has found a lane within three entries of it.  These tests put a tree that is
much deeper than the LDS part under caps of 4, 8 and 21 entries (cap 4: most waves really spill, so one wave switches between the two
forms many times), with and without the camera rays' candidate lists (their set-up pushes three entries unchecked), and compare every
image bit for bit with a render whose whole stack is in LDS and with the oracle.  Sample and bounce counters share a register: the
largest counts the host hands to k_stream are rendered against the oracle.  A CPU test reads the registers, scratch and occupancy of
every non-counting instantiation from the code object (tools/kernel_resources.py).  rt_stats.lastKernel says which kernel ran; nothing
in rt_stats says whether a launch had a global stack part, so the no-spill case rests on the host's rule (rt_render.hip plan_launch: a
global part exactly when bvhMaxStack + 3 exceeds the LDS part) and the statistic it reads."""
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import assert_bitwise, run_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

W, H = 64, 48
CROP = (16, 12, 48, 36)             # the oracle's share of a frame (x0, y0, x1, y1): its flat loop over ~2,000 triangles is the slow part
FULL_LDS = 128                      # stream_stack at which the deep scene's whole stack is in LDS


def deep_scene(rtx, rays=4, bounces=8):
    """~2,000 triangles whose BVH is far deeper than a balanced one: a strip of 120 thin triangles whose length and distance from its
    start grow by 10 % from one to the next (5 mm to 360 m: the split search peels them off one by one), in front of a cluster of
    finely tessellated spheres, over the small mixed scene of the parity tests."""
    h = rtx.host
    m = rtx.scenes.mesh_test_scene(W, H)
    m.numRaysPerPixel, m.maxBounceCount = rays, bounces
    tri = np.zeros(120, rtx.TRIANGLE)
    s = np.float32(0.004) * np.float32(1.1) ** np.arange(120, dtype=np.float32)
    y, z = np.float32(0.25), np.float32(-1.5)
    zero = np.zeros_like(s)
    tri["posA"] = np.stack([s - 4, zero + y, zero + z], 1)
    tri["posB"] = np.stack([s - 4, y + np.float32(0.02) * s + np.float32(0.01), zero + z], 1)      # (A, B, C wound to face the camera at -z)
    tri["posC"] = np.stack([s * np.float32(1.078) - 4, zero + y, zero + z], 1)
    tri["normalA"] = tri["normalB"] = tri["normalC"] = (0, 0, -1)
    white = (1, 1, 1, 1)
    m.meshes.append(h.RayTracedMesh(h.Transform(), [h.RayTracingMaterial(colour=(0.9, 0.7, 0.2, 1), emissionColour=(0, 0, 0, 0), specularColour=white,
                                                                            specularProbability=0.0)], rtx.scenes.chunked(tri)))
    ball = rtx.scenes.uv_sphere_triangles(16, 24)
    for k, (pos, r) in enumerate((((-1.2, 0.9, 0.5), 0.9), ((1.4, 0.6, -0.5), 0.6))):
        m.meshes.append(h.RayTracedMesh(h.Transform(position=pos, lossyScale=(r, r, r)),
                                        [h.RayTracingMaterial(colour=(0.3 + 0.5 * k, 0.8, 0.9 - 0.5 * k, 1), emissionColour=(0, 0, 0, 0), specularColour=white,
                                                              smoothness=0.9, specularProbability=0.5 * k)], rtx.scenes.chunked(ball, 40)))
    return m


def crop(img):
    x0, y0, x1, y1 = CROP
    return np.ascontiguousarray(img[y0:y1, x0:x1])


def render_with(tracer, buffers, frames=2, **options):
    """(accum, last frame, stats) of k_stream with the given options; the options are back at their defaults afterwards"""
    defaults = {"stream_stack": 0, "primary_lists": 1, "compact_nodes": 1}
    for k, v in options.items():
        tracer.set_option(k, v)
    try:
        acc, last = run_gpu(tracer, buffers, 0, frames, kernel=1)
        st = tracer.stats()
    finally:
        for k in options:
            tracer.set_option(k, defaults[k])
    return acc, last, st


@pytest.fixture(scope="module")
def deep(rtx, oracle, tracer):
    """the deep scene, its render with the whole stack in LDS, and the oracle's crop: computed once, never changed"""
    b = deep_scene(rtx).build_buffers()
    acc, last, st = render_with(tracer, b, stream_stack=FULL_LDS)
    want, want_last, cnt = oracle.render(*b, 0, 2, rect=CROP)
    for a in (acc, last, want, want_last):
        a.setflags(write=False)
    return dict(buffers=b, acc=acc, last=last, stats=st, want=want, want_last=want_last)


@gpu
def test_the_scene_is_deep_and_the_plain_path_alone_renders_it(deep):
    """No spill part at all (the BVH's worst case fits the LDS part: k_stream gets no global stack): the plain pushes and pops alone
    == the oracle."""
    st = deep["stats"]
    assert 1800 <= st["numTriangles"] <= 2300, st["numTriangles"]
    print(f"deep scene: {st['numTriangles']} triangles, bvhMaxStack {st['bvhMaxStack']}")
    assert st["bvhMaxStack"] + 3 <= FULL_LDS                 # rt_render.hip plan_launch: a global stack only when the worst case + 3 exceeds the LDS part
    assert st["bvhMaxStack"] + 3 >= 21 + 6                   # ... and far beyond the product's 21 entries
    assert_bitwise(crop(deep["last"]), deep["want_last"], "whole stack in LDS vs oracle, last frame")
    assert_bitwise(crop(deep["acc"]), deep["want"], "whole stack in LDS vs oracle, accum")


@gpu
@pytest.mark.parametrize("primary_lists", [0, 1])
@pytest.mark.parametrize("cap", [4, 8, 21])
def test_deep_tree_against_a_small_lds_part(tracer, deep, cap, primary_lists):
    acc, last, st = render_with(tracer, deep["buffers"], stream_stack=cap, primary_lists=primary_lists)
    assert st["bvhMaxStack"] + 3 > cap
    assert st["rays"] == deep["stats"]["rays"]
    what = f"stream_stack {cap}, primary_lists {primary_lists}"
    assert_bitwise(last, deep["last"], what + " vs whole stack in LDS, last frame")
    assert_bitwise(acc, deep["acc"], what + " vs whole stack in LDS, accum")
    assert_bitwise(crop(last), deep["want_last"], what + " vs oracle, last frame")
    assert_bitwise(crop(acc), deep["want"], what + " vs oracle, accum")


@gpu
def test_f32_node_instantiation_with_a_spilling_stack(tracer, deep):
    acc, last, st = render_with(tracer, deep["buffers"], stream_stack=8, compact_nodes=0)
    assert_bitwise(last, deep["last"], "compact_nodes 0, stream_stack 8, last frame")
    assert_bitwise(acc, deep["acc"], "compact_nodes 0, stream_stack 8, accum")


@gpu
def test_philox_instantiation_with_a_spilling_stack(rtx, oracle, tracer):
    params, spheres, tris, infos = deep_scene(rtx).build_buffers()
    params = params.copy(); params["rngMode"] = 1
    b = (params, spheres, tris, infos)
    acc, last, st = render_with(tracer, b, frames=1, stream_stack=8)
    full, full_last, _ = render_with(tracer, b, frames=1, stream_stack=FULL_LDS)
    want, want_last, cnt = oracle.render(*b, 0, 1, rect=CROP)
    assert_bitwise(last, full_last, "philox, stream_stack 8 vs whole stack in LDS")
    assert_bitwise(crop(last), want_last, "philox, stream_stack 8 vs oracle")


def mirror_room_with_a_mesh(rtx):
    """config2's spheres as white mirrors (Russian roulette's p = 1: only the loop bound ends a path) and one cube, so that the scene has
    a BVH and runs the triangle instantiation"""
    h = rtx.host
    m = rtx.scenes.config2(8, 8)
    for s in m.spheres:
        s.material.colour = (1, 1, 1, 1); s.material.specularColour = (1, 1, 1, 1); s.material.emissionStrength = 0.0
        s.material.specularProbability = 1.0; s.material.smoothness = 1.0; s.material.flag = 0
    m.meshes.append(h.RayTracedMesh(h.Transform(position=(0.0, 0.5, 0.0)),
                                    [h.RayTracingMaterial(colour=(1, 1, 1, 1), emissionColour=(0, 0, 0, 0), specularColour=(1, 1, 1, 1),
                                                          smoothness=1.0, specularProbability=1.0)], rtx.scenes.chunked(rtx.scenes.cube_triangles())))
    return m


@gpu
@pytest.mark.parametrize("rays,bounces", [(1, 32000), (65000, 1)], ids=["32000 bounces", "65000 rays"])
def test_pcg_at_the_largest_counts_k_stream_takes(rtx, oracle, tracer, rays, bounces):
    """Sample and bounce share a register (sample | bounce << 16): the host gives k_stream at most 65000 rays per pixel and 32000
    bounces, so that the packed counter never reaches the sign bit.  8x8 pixels at each maximum: image and ray count == oracle."""
    m = mirror_room_with_a_mesh(rtx)
    m.numRaysPerPixel, m.maxBounceCount = rays, bounces
    b = m.build_buffers()
    acc, last = run_gpu(tracer, b, 0, 1, kernel=1)
    st = tracer.stats()
    want, want_last, cnt = oracle.render(*b, 0, 1)
    assert st["numBvhNodes"] > 0 and st["lastKernel"] == 1, st["lastKernel"]          # k_stream itself ran, not the fallback
    if bounces == 32000:
        assert cnt["rays"] > 32 * 32001                      # paths did run into the loop bound
    assert st["rays"] == cnt["rays"]
    assert_bitwise(last, want_last, f"pcg, {rays} rays, {bounces} bounces")


@gpu
@pytest.mark.parametrize("rays,bounces", [(1, 32001), (65001, 0)], ids=["32001 bounces", "65001 rays"])
def test_pcg_counts_above_the_limit_go_to_the_tile_kernel(rtx, oracle, tracer, rays, bounces):
    """One more than k_stream takes: the frame is k_trace's even when k_stream is asked for (include/rt.h, option "kernel"), and equals the
    oracle all the same."""
    m = mirror_room_with_a_mesh(rtx)
    m.numRaysPerPixel, m.maxBounceCount = rays, bounces
    b = m.build_buffers()
    acc, last = run_gpu(tracer, b, 0, 1, kernel=1)
    st = tracer.stats()
    assert st["lastKernel"] == 0, st["lastKernel"]
    want, want_last, cnt = oracle.render(*b, 0, 1)
    assert st["rays"] == cnt["rays"]
    assert_bitwise(last, want_last, f"pcg above the limit, {rays} rays, {bounces} bounces")


def claimed_waves(count, philox, h, tri):
    """rt_stream.hpp stream_waves(), with the header's own RT_STREAM_WAVES / RT_STREAM_WAVES_PHILOX defaults (what the product build compiles)"""
    import re
    text = open(os.path.join(ROOT, "ray-tracing-extended_amd", "csrc", "rt_stream.hpp")).read()
    pcg = int(re.search(r"#define RT_STREAM_WAVES (\d+)", text).group(1))
    phx = int(re.search(r"#define RT_STREAM_WAVES_PHILOX (\d+)", text).group(1))
    return 3 if count else 6 if not tri else phx if philox else 5 if not h else pcg


# The one instantiation that ships with scratch, as it did before this file existed: the Philox sphere-only k_stream at six waves keeps
# one spilled VGPR (8 B) and was measured with it against five waves (rt_stream.hpp: 32.6 -> 35.1 Grays/s).  Its figures are pinned: any
# other scratch anywhere, or more of it here, fails.
KNOWN_SCRATCH = {"void rtk::k_stream<false, true, false, false>": dict(ScratchSize=8, spills=1, VGPRs=80)}


def test_code_object_has_the_registers_scratch_and_occupancy_stream_waves_claims():
    """Every non-counting k_stream / k_cam_stream instantiation: no scratch, the occupancy stream_waves() asks for, and no more VGPRs
    than that occupancy allows (512 per SIMD lane, allocated in blocks of 8).  Figures as the compiler reports them for the code object."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.table("rt_stream_kernels.hip")
    seen = 0
    for r in rows:
        m = re.match(r"void rtk::k_stream<(\w+), (\w+), (\w+), (\w+)>", r["name"])
        c = re.match(r"void rtk::k_cam_stream<(\w+), (\w+), (\w+)>", r["name"])
        if m:
            count, philox, h, tri = (a == "true" for a in m.groups())
        elif c:
            count = False
            philox, h, tri = (a == "true" for a in c.groups())
        else:
            continue
        if count:
            continue
        waves = claimed_waves(count, philox, h, tri)
        print(f"{r['name']}: VGPRs {r['VGPRs']}, scratch {r['ScratchSize']} B, occupancy {r['Occupancy']} (claimed {waves})")
        known = KNOWN_SCRATCH.get(r["name"])
        if known:
            assert (r["ScratchSize"], r["VGPRs Spill"], r["VGPRs"]) == (known["ScratchSize"], known["spills"], known["VGPRs"]), r
        else:
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
        assert r["Occupancy"] == waves, r
        assert r["VGPRs"] <= (512 // waves) // 8 * 8, r
        seen += 1
    assert seen == 6 + 6                                     # k_stream: PCG / Philox x f32 / f16 nodes + two sphere-only; the same six k_cam_stream
