"""The feature buffers on the GPU (rt_render_aov and its rt_multi form): both planes bitwise against tests/aov_oracle.c, every pixel and
channel, on the reference's scenes for every sub-stream layout (N = 1, 3: one lane per pixel; 4: four; 16, 20, 64: sixteen), both
intersect modes, both BVH builders and node forms, depth of field, accumulation, strips, bands and several contexts, moved local meshes,
scenes without triangles or without anything — and the image path next to it, undisturbed."""
import ctypes
import os

import numpy as np
import pytest

import aov_check
from aov_check import assert_same_bits
from test_aov_cpu import emissive_scene
from test_gpu_scenes import GOLDEN

W, H = 160, 90
SCENES = ["Balls_Outdoors", "Chess", "Knight", "Reflective_Balls", "Suzanne", "Thumbnail", "mesh_test_scene"]
pytestmark = pytest.mark.gpu


def scene_of(rtx, name, w=W, h=H):
    from rtx_amd import unity_scene
    if name == "mesh_test_scene":
        return rtx.scenes.mesh_test_scene(w, h)
    return unity_scene.load_scene_npz(os.path.join(GOLDEN, "scenes", name + ".npz"), w, h)


def loaded(rtx, buffers, **options):
    params, spheres, tris, infos = buffers
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    return t


def planes(t):
    return t.read_aov(0), t.read_aov(1)


def check(rtx, t, buffers, frames, what, rect=None):
    want = aov_check.oracle_planes(rtx, *buffers, frames, rect)
    for g, w_, name in zip(planes(t), want, ("albedo / coverage", "normal / depth")):
        assert_same_bits(g, w_, f"{what}: {name}")
    return want


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 16, 20, 64])
@pytest.mark.parametrize("name", SCENES)
def test_reference_scenes(rtx, name, n, mode):
    mgr = scene_of(rtx, name)
    mgr.numRaysPerPixel = n
    buffers = mgr.build_buffers()
    buffers[0]["intersectMode"] = mode
    with loaded(rtx, buffers) as t:
        t.render_aov(2, 1)
        want = check(rtx, t, buffers, [2], f"{name} N {n} mode {mode}")
        info = t.aov_info()
        assert info["framesAccumulated"] == 1 and info["lastSampleLanes"] == (16 if n >= 16 else 4 if n >= 4 else 1)
        assert info["lastKernelMs"] > 0
    assert (want[0][..., 3] > 0).any()


@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("name", ["Chess", "mesh_test_scene"])
def test_builders_and_node_forms(rtx, name, device_bvh, compact_nodes):
    mgr = scene_of(rtx, name)
    mgr.numRaysPerPixel = 16
    buffers = mgr.build_buffers()
    with loaded(rtx, buffers, device_bvh=device_bvh, compact_nodes=compact_nodes) as t:
        t.render_aov(0, 2)
        check(rtx, t, buffers, [0, 1], f"{name} device_bvh {device_bvh} compact_nodes {compact_nodes}")
        assert t.stats()["bvhBuiltOnDevice"] == device_bvh


def test_small_lds_stack_spills_to_the_overflow_area(rtx):
    mgr = scene_of(rtx, "Chess", 64, 36)
    mgr.numRaysPerPixel = 4
    buffers = mgr.build_buffers()
    with loaded(rtx, buffers, lds_stack=3) as t:
        t.render_aov(0, 1)
        check(rtx, t, buffers, [0], "lds_stack 3")
        assert t.stats()["bvhMaxStack"] > 3


@pytest.mark.parametrize("n", [4, 64])
def test_depth_of_field(rtx, n):
    mgr = rtx.scenes.chess_instanced(1, W, H, dof=True)
    mgr.numRaysPerPixel = n
    buffers = mgr.build_buffers()
    assert buffers[0]["defocusStrength"] > 0
    with loaded(rtx, buffers) as t:
        t.render_aov(5, 1)
        want = check(rtx, t, buffers, [5], f"depth of field N {n}")
    c = want[0][..., 3]
    assert ((c > 0) & (c < 1)).any()


def test_chess_light_is_passed_through(rtx):
    """the reference scene's InvisibleLight quad, looked at from below: the planes show what lies behind it"""
    mgr = rtx.scenes.chess_instanced(1, 64, 36)
    mgr.numRaysPerPixel = 4
    buffers = mgr.build_buffers()
    assert (buffers[3]["material"]["flag"] == 2).any()
    for bounces in (0, 1, 8):
        buffers[0]["maxBounceCount"] = bounces
        with loaded(rtx, buffers) as t:
            t.render_aov(0, 1)
            check(rtx, t, buffers, [0], f"chess, maxBounceCount {bounces}")


def test_rng_modes_give_identical_planes(rtx):
    buffers = scene_of(rtx, "mesh_test_scene").build_buffers()
    got = []
    for mode in (0, 1):
        buffers[0]["rngMode"] = mode
        with loaded(rtx, buffers) as t:
            t.render_aov(0, 2)
            got.append(planes(t))
            if mode == 1:
                check(rtx, t, buffers, [0, 1], "Philox mode")
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 4, 16, 20, 64])
def test_coverage_is_the_rendered_image_of_an_all_emissive_scene(rtx, n):
    """tests/test_aov_cpu.py case (a) on the device: rt_render in Philox mode against the coverage plane"""
    buffers = emissive_scene(rtx, n, width=W, height=H)
    with loaded(rtx, buffers) as t:
        t.render_frame(3)
        image = t.read_last_frame()
        t.render_aov(3, 1)
        c = t.read_aov(0)[..., 3]
    want = np.stack([c, np.float32(0.5) * c, np.float32(0.25) * c, np.ones_like(c)], -1)
    assert_same_bits(image, want, f"N = {n}")
    assert (c == 0).any() and (c == 1).any()


def test_accumulation_in_one_call_or_two(rtx):
    mgr = scene_of(rtx, "mesh_test_scene")
    mgr.numRaysPerPixel = 16
    buffers = mgr.build_buffers()
    with loaded(rtx, buffers) as t:
        t.render_aov(0, 4)
        one = planes(t)
        check(rtx, t, buffers, [0, 1, 2, 3], "four frames")
        assert t.aov_info()["framesAccumulated"] == 4
        t.reset_aov()
        assert t.aov_info()["framesAccumulated"] == 0 and not t.read_aov(0).any() and not t.read_aov(1).any()
        t.render_aov(0, 2)
        t.render_aov(2, 2)
        for a, b in zip(one, planes(t)):
            assert a.tobytes() == b.tobytes()
        t.render_aov(9, 0)                                  # nothing
        assert t.aov_info()["framesAccumulated"] == 4
    assert (one[1][..., :3] < 0).any() and (one[1][..., 3] > 1).any()          # signed normals, depths beyond 1: nothing is saturated


def test_rows_bands_and_several_contexts(rtx):
    mgr = scene_of(rtx, "mesh_test_scene", 100, 75)         # 75 rows: a partial last band, 100 columns: partial tiles
    mgr.numRaysPerPixel = 16
    buffers = mgr.build_buffers()
    with loaded(rtx, buffers) as t:
        t.render_aov(1, 2)
        full = check(rtx, t, buffers, [1, 2], "whole image")
        t.set_rows(13, 31)
        assert not t.read_aov(0).any()                      # a new strip: new, zeroed planes
        t.render_aov(1, 2)
        for g, w_ in zip(planes(t), full):
            assert g.tobytes() == w_[13:44].tobytes()
        t.set_bands(1, 3)
        t.render_aov(1, 2)
        rows = np.concatenate([np.arange(y, min(y + 8, 75)) for y in range(8, 75, 24)])
        for g, w_ in zip(planes(t), full):
            assert g.tobytes() == w_[rows].tobytes()
    for n_ctx in (2, 3):
        with rtx.MultiTracer([0] * n_ctx) as m:
            m.set_params(buffers[0])
            m.upload(spheres=buffers[1], triangles=buffers[2], meshinfo=buffers[3])
            m.render_aov(1, 1)
            m.render_aov(2, 1)
            for which in (0, 1):
                assert m.read_aov(which).tobytes() == full[which].tobytes(), (n_ctx, which)
            assert [i["framesAccumulated"] for i in m.aov_info()] == [2] * n_ctx
            assert m.info()["bvhBuilds"] == 1
            m.reset_aov()
            assert not m.read_aov(0).any()
            m.set_option("peer_copies", 1)
            m.render_aov(1, 2)
            assert m.read_aov(1).tobytes() == full[1].tobytes()


def test_local_meshes_after_new_transforms(rtx):
    mgr = rtx.scenes.mesh_test_scene(W, H)
    mgr.numRaysPerPixel = 4
    params, spheres, _, _ = mgr.build_buffers()
    ltris, chunks = mgr.build_local_buffers()
    xf = mgr.build_transforms()
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres)
        t.upload_local_meshes(ltris, chunks, len(mgr.meshes))
        t.set_mesh_transforms(xf)
        t.render_aov(0, 1)                                  # builds the scene
        world, infos = t.read_world_geometry()
        check(rtx, t, (params, spheres, world, infos), [0], "local meshes")
        xf2 = xf.copy()
        xf2["position"] += np.float32(0.75)
        xf2["rotation"][:, 1] = np.float32(0.2)
        xf2["rotation"][:, 3] = np.float32(np.sqrt(1 - 0.04))
        t.set_mesh_transforms(xf2)
        t.reset_aov()
        t.render_aov(0, 1)                                  # the geometry pass, then the feature frame
        world2, infos2 = t.read_world_geometry()
        assert world2.tobytes() != world.tobytes()
        check(rtx, t, (params, spheres, world2, infos2), [0], "local meshes, moved")


def test_spheres_only_and_empty_scene(rtx):
    mgr = scene_of(rtx, "Balls_Outdoors")
    buffers = mgr.build_buffers()
    assert len(buffers[2]) == 0
    with loaded(rtx, buffers) as t:
        t.render_aov(0, 1)
        check(rtx, t, buffers, [0], "spheres only")
    params = buffers[0]
    with rtx.Tracer(0) as t:                                # nothing uploaded
        t.set_params(params)
        t.render_aov(0, 3)
        assert t.aov_info()["framesAccumulated"] == 3
        for p in planes(t):
            assert p.shape == (H, W, 4) and not p.view(np.uint32).any()


def test_resize_zeroes_the_planes_and_reset_accum_does_not(rtx):
    buffers = scene_of(rtx, "mesh_test_scene").build_buffers()
    with loaded(rtx, buffers) as t:
        t.render(0, 1)
        t.render_aov(0, 2)
        before = planes(t)
        assert before[0].any()
        t.reset_accum()
        assert not t.read_accum().any()
        for a, b in zip(before, planes(t)):
            assert a.tobytes() == b.tobytes()
        assert t.aov_info()["framesAccumulated"] == 2
        small = buffers[0].copy()
        small["width"], small["height"] = 80, 45
        t.set_params(small)
        for p in planes(t):
            assert p.shape == (45, 80, 4) and not p.any()
        assert t.aov_info()["framesAccumulated"] == 0
        t.render_aov(0, 1)
        check(rtx, t, (small,) + tuple(buffers[1:]), [0], "after the resize")


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_the_image_path_is_undisturbed(rtx, rng_mode):
    buffers = scene_of(rtx, "mesh_test_scene").build_buffers()
    buffers[0]["rngMode"] = rng_mode

    def run(with_features, queued):
        with loaded(rtx, buffers, kernel=1) as t:           # (one kernel for both runs: the automatic choice goes by measured times)
            rays = []
            if with_features:
                t.render_aov(0, 1)                          # builds the scene before the first frame
            for f in range(4):
                if queued:
                    t.submit_frame(f)
                    t.submit_frame(f + 4)
                else:
                    t.render(f, 1)
                    rays.append(t.stats()["rays"])
                if with_features:
                    t.render_aov(f, 1)                      # settles the queue first
            if queued:
                t.wait()
            st = t.stats()
            return t.read_accum(), t.read_last_frame(), st["numRenderedFrames"], rays, (planes(t) if with_features else None)

    for queued in (False, True):
        a = run(False, queued)
        b = run(True, queued)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), queued
        assert a[2] == b[2] == (8 if queued else 4) and a[3] == b[3]
        want = aov_check.oracle_planes(rtx, *buffers, [0, 0, 1, 2, 3])
        for g, w_ in zip(b[4], want):
            assert_same_bits(g, w_, f"interleaved with frames, queued {queued}")


def hip_runtime():
    """the HIP runtime the library itself has loaded (its path from the process's mappings), for a device buffer of the test's own"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert paths, "the tracer library has not loaded a HIP runtime"
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


def test_copy_to_device_and_error_codes(rtx):
    buffers = scene_of(rtx, "mesh_test_scene", 64, 48).build_buffers()
    lib = rtx.load_library()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
    buf = np.zeros(64 * 48 * 4, np.float32)
    assert lib.rt_render_aov(None, 0, 1) == -1 and lib.rt_read_aov(None, 0, fp(buf), buf.size) == -1
    assert lib.rt_reset_aov(None) == -1 and lib.rt_get_aov_info(None, None) == -1 and lib.rt_copy_aov_to_device(None, 0, None, 0) == -1
    assert lib.rt_multi_render_aov(None, 0, 1) == -1 and lib.rt_multi_read_aov(None, 0, fp(buf), buf.size) == -1 and lib.rt_multi_reset_aov(None) == -1
    with rtx.Tracer(0) as t:
        c = t._ctx
        assert lib.rt_render_aov(c, 0, 1) == -2 and b"rt_set_params" in lib.rt_last_error(c)
        assert lib.rt_read_aov(c, 0, fp(buf), buf.size) == -2
        t.set_params(buffers[0])
        t.upload(spheres=buffers[1], triangles=buffers[2], meshinfo=buffers[3])
        assert lib.rt_render_aov(c, 0, -1) == -2 and b"n_frames" in lib.rt_last_error(c)
        assert lib.rt_render_aov(c, 0, 0) == 0
        assert lib.rt_render_aov(c, 0, 1) == 0
        for which in (-1, 2):
            assert lib.rt_read_aov(c, which, fp(buf), buf.size) == -2 and b"plane" in lib.rt_last_error(c)
        assert lib.rt_read_aov(c, 0, fp(buf), buf.size - 4) == -2 and b"expected" in lib.rt_last_error(c)
        assert lib.rt_read_aov(c, 0, None, buf.size) == -2
        assert lib.rt_get_aov_info(c, None) == -2
        assert lib.rt_read_aov(c, 1, fp(buf), buf.size) == 0
        hip, dev, back = hip_runtime(), ctypes.c_void_p(), np.zeros_like(buf)
        assert hip.hipMalloc(ctypes.byref(dev), buf.nbytes) == 0
        try:
            t.copy_aov_to_device(1, dev.value, buf.size)
            assert hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), dev, buf.nbytes, 2) == 0       # device to host
        finally:
            hip.hipFree(dev)
        assert back.tobytes() == buf.tobytes() and buf.any()
        assert lib.rt_copy_aov_to_device(c, 1, None, buf.size) == -2
    with rtx.MultiTracer([0, 0]) as m:
        assert lib.rt_multi_render_aov(m._m, 0, 1) == -2
        m.set_params(buffers[0])
        m.upload(spheres=buffers[1], triangles=buffers[2], meshinfo=buffers[3])
        assert lib.rt_multi_render_aov(m._m, 0, -1) == -2 and lib.rt_multi_render_aov(m._m, 0, 0) == 0
        assert lib.rt_multi_read_aov(m._m, 2, fp(buf), buf.size) == -2
        assert lib.rt_multi_read_aov(m._m, 0, fp(buf), 8) == -2
        assert lib.rt_multi_read_aov(m._m, 0, None, buf.size) == -2


def test_headline_frame_against_the_oracle(rtx):
    """one whole 1920 x 1080 feature frame of the headline workload (configuration 3: 100k triangles, 64 rays per pixel)"""
    mgr = rtx.scenes.config3()
    buffers = mgr.build_buffers()
    assert (buffers[0]["width"], buffers[0]["height"], buffers[0]["numRaysPerPixel"]) == (1920, 1080, 64)
    with loaded(rtx, buffers) as t:
        t.render_aov(0, 1)
        got = planes(t)
        info = t.aov_info()
    print(f"headline feature frame: {info['lastKernelMs']:.3f} ms, {info['lastSampleLanes']} lanes per pixel")
    want = aov_check.oracle_planes(rtx, *buffers, [0])
    for g, w_, name in zip(got, want, ("albedo / coverage", "normal / depth")):
        assert_same_bits(g, w_, "headline: " + name)
