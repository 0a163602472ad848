"""Radiance queries on the GPU (rt_trace_radiance and its device and rt_multi forms): every float of every result bitwise against the
checker (tests/query_oracle.c: the oracle's own trace() per ray and sample) and, with no checker in between, against the frame
kernel in Philox mode; invisible slicing, rt_multi, a spilling traversal stack, far origins, the device entry; a call leaves every
other state of the context alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import query_check as rc
from ray_query_helpers import SCENES, camera_rays, make_rays, random_rays, scene_of
from test_gpu_ray_query import far_rays, loaded_tracer, local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def check(rtx, tracer, params, spheres, tris, infos, rays, samples, what, seed=0, first_index=0):
    """rays on `tracer` (which holds the scene and params) against the checker; returns the result"""
    want = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, samples, seed, first_index)
    got = tracer.trace_radiance(rays, samples, seed, first_index)
    rc.assert_same_bits(got, want, what)
    return got


def light_manager(rtx):
    """mesh_test_scene with every fourth object an emitting InvisibleLight: spheres, triangles, a checker floor, pass-through casts"""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    for i, mesh in enumerate(mgr.meshes[2:]):
        if i % 4 == 0:
            for mat in mesh.materials:
                mat.flag = rtx.MaterialFlag.InvisibleLight
                mat.emissionColour, mat.emissionStrength = (1.0, 0.8, 0.6, 1.0), 2.0
    return mgr


@pytest.fixture(scope="module")
def light_scene(rtx):
    """the scene most tests share, its camera rays, and the checker's answers by (samples, maxBounceCount), computed once"""
    mgr = light_manager(rtx)
    params, spheres, tris, infos = mgr.build_buffers()
    assert (infos["material"]["flag"] == 2).any()
    rays = camera_rays(rtx, params)
    cache = {}

    def want(samples, bounces):
        if (samples, bounces) not in cache:
            p = params.copy()
            p["maxBounceCount"] = bounces
            cache[samples, bounces] = rc.oracle_radiance(rtx, p, spheres, tris, infos, rays, samples, seed=7, first_index=11)
            cache[samples, bounces].setflags(write=False)
        return cache[samples, bounces]
    return mgr, params, spheres, tris, infos, rays, want


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SCENES + ["mesh_test_scene"])
def test_camera_rays_of_the_reference_scenes(rtx, name, mode):
    t, params, s, tr, mi = loaded_tracer(rtx, scene_of(rtx, name), mode)
    with t:
        got = check(rtx, t, params, s, tr, mi, camera_rays(rtx, params), 21, f"{name} mode {mode}", seed=1)
        assert (got[:, 3] == 1).all() and len(np.unique(got[:, :3], axis=0)) > 16
        assert t.radiance_info()["lastSampleLanes"] == 16


@pytest.mark.parametrize("samples", [1, 3, 4, 16, 64])
def test_sample_counts_and_batch_sizes(rtx, light_scene, samples):
    mgr, params, s, tr, mi, rays, want = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        full = want(samples, int(params["maxBounceCount"]))
        for n in (1, 5, 67, 3072):
            # (a batch of the first n rays has the stream indices of the whole batch's first n)
            got = t.trace_radiance(rays[:n], samples, seed=7, first_index=11)
            rc.assert_same_bits(got, full[:n], f"samples {samples}, n {n}")
        assert t.radiance_info()["lastSampleLanes"] == (16 if samples >= 16 else 4 if samples >= 4 else 1)
        assert t.radiance_info()["samples"] == samples


@pytest.mark.parametrize("bounces", [0, 1, 8])
@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_node_forms_builders_and_bounce_limits(rtx, light_scene, compact_nodes, device_bvh, bounces):
    mgr, params, s, tr, mi, rays, want = light_scene
    p = params.copy()
    p["maxBounceCount"] = bounces
    with rtx.Tracer(0) as t:
        t.set_option("compact_nodes", compact_nodes)
        t.set_option("device_bvh", device_bvh)
        t.set_params(p)
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        got = t.trace_radiance(rays, 16, seed=7, first_index=11)
        rc.assert_same_bits(got, want(16, bounces), f"compact_nodes {compact_nodes} device_bvh {device_bvh} bounces {bounces}")


@pytest.mark.parametrize("mode", [0, 1])
def test_random_rays_directions_bounds_and_special_values(rtx, light_scene, mode):
    mgr, *_ = light_scene
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, mode)
    with t:
        rays = random_rays(rtx, tr, s, 1536, seed=11 + mode)          # unnormalised, axis-aligned and zero directions; inside and outside
        rays["tMax"][1::4] = np.float32(6.0)                         # a finite bound: some first hits lie beyond it
        rays["tMax"][2::16] = np.float32(0.0)
        rays["tMax"][6::16] = np.float32(np.nan)
        got = check(rtx, t, params, s, tr, mi, rays, 5, f"random rays mode {mode}", seed=2, first_index=0xFFFFFF00)
        assert (got[2::16] == 0).all() and (got[6::16] == 0).all() and (got[:, 3] == 1).any()
        unbounded = rays.copy()
        unbounded["tMax"] = np.inf
        free = t.trace_radiance(unbounded, 5, seed=2, first_index=0xFFFFFF00)
        assert (free[1::4] != got[1::4]).any()                          # (the bound changed some answers)
        # NaN / inf origins and directions: whatever the arithmetic gives, the checker's bits, and no fault
        o, d = np.asarray(rays["origin"][:64]).copy(), np.asarray(rays["direction"][:64]).copy()
        o[:8, 0], o[8:16, 1], o[16:24, 2] = np.nan, np.inf, -np.inf
        d[24:32, 0], d[32:40, 1], d[40:48] = np.nan, np.inf, 0.0
        check(rtx, t, params, s, tr, mi, make_rays(rtx, o, d), 4, f"NaN / inf / zero mode {mode}")


@pytest.mark.parametrize("defocus", [0.0, 30.0])
def test_the_frame_kernel_traces_the_same_radiance(rtx, light_scene, defocus):
    """Philox mode, one ray per pixel: frame f == the radiance along sample 0's camera rays with seed f (k_stream against k_radiance)"""
    mgr, params, s, tr, mi, *_ = light_scene
    p = params.copy()
    p["rngMode"], p["numRaysPerPixel"], p["defocusStrength"] = 1, 1, defocus
    with rtx.Tracer(0) as t:
        t.set_params(p)
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        for f in (0, 6):
            t.render_frame(f)
            frame = t.read_last_frame()
            got = t.trace_radiance(rc.frame_camera_rays(rtx, p, f), 1, seed=f)
            rc.assert_same_bits(got, frame.reshape(-1, 4), f"frame {f}, defocus {defocus}")
            assert len(np.unique(got[:, :3], axis=0)) > 16


def test_slices_and_split_calls_are_invisible(rtx, light_scene):
    mgr, params, s, tr, mi, rays, want = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        r = rays[:1000]
        whole = t.trace_radiance(r, 5, seed=7, first_index=11)
        rc.assert_same_bits(whole, want(5, int(params["maxBounceCount"]))[:1000], "default slice")
        t.set_option("radiance_slice", 100)
        rc.assert_same_bits(t.trace_radiance(r, 5, seed=7, first_index=11), whole, "radiance_slice 100")
        t.set_option("radiance_slice", 333)
        rc.assert_same_bits(t.trace_radiance(r, 5, seed=7, first_index=11), whole, "radiance_slice 333")
        t.set_option("radiance_slice", 1 << 22)
        a = t.trace_radiance(r[:377], 5, seed=7, first_index=11)
        b = t.trace_radiance(r[377:], 5, seed=7, first_index=11 + 377)
        rc.assert_same_bits(np.concatenate([a, b]), whole, "two calls")


def test_multi_tracer_gives_the_single_context_bits(rtx, light_scene):
    mgr, params, s, tr, mi, rays, want = light_scene
    with rtx.MultiTracer([0] * 3) as m:
        m.set_params(params)
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        got = m.trace_radiance(rays[:2999], 16, seed=7, first_index=11)
        rc.assert_same_bits(got, want(16, int(params["maxBounceCount"]))[:2999], "three contexts")


def test_multi_tracer_on_local_meshes_after_new_transforms(rtx):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    t, params, s, world, infos, _ = local_tracer(rtx, mgr)
    rays = np.concatenate([random_rays(rtx, world, s, 1200, seed=15), far_rays(rtx, world, 100, 1e5, seed=16)])
    with t:
        single = check(rtx, t, params, s, world, infos, rays, 4, "local meshes, one context", seed=5)
    xf = mgr.build_transforms()
    xf["position"] += np.float32(0.5)
    with rtx.MultiTracer([0] * 3) as m:
        m.set_params(params)
        m.upload(spheres=s)
        m.upload_local_meshes(*mgr.build_local_buffers(), len(mgr.meshes))
        m.set_mesh_transforms(xf)
        rc.assert_same_bits(m.trace_radiance(rays, 4, seed=5), single, "local meshes, three contexts")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, compact_nodes):
    """three stack entries per lane in LDS, the rest of the Knight's tree in the global overflow area (both node forms)"""
    mgr = scene_of(rtx, "Knight")
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes)
    with t:
        rays = camera_rays(rtx, params, 48, 32)
        got = check(rtx, t, params, s, tr, mi, rays, 16, f"lds_stack 3 compact_nodes {compact_nodes}")
        assert t.stats()["bvhMaxStack"] > 3         # (the overflow area was in use)
    t, *_ = loaded_tracer(rtx, mgr, 0, compact_nodes=compact_nodes)
    with t:
        rc.assert_same_bits(t.trace_radiance(rays, 16), got, "against the whole stack in LDS")


def test_far_origins_widen_the_padding(rtx, light_scene):
    mgr, params, s, tr, mi, *_ = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        check(rtx, t, params, s, tr, mi, random_rays(rtx, tr, s, 256, seed=3), 4, "near")
        repads = t.stats()["bvhRepads"]
        got = check(rtx, t, params, s, tr, mi, far_rays(rtx, tr, 512, 1e5, seed=9), 4, "origins 1e5 away")
        assert t.stats()["bvhRepads"] > repads
        assert len(np.unique(got[:, :3], axis=0)) > 16


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/radiance_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "radiance_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "radiance device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


STATS_MAY_MOVE = ("bvhBuilds", "bvhRebuilds", "bvhRepads")


def test_a_call_moves_no_other_state(rtx, light_scene):
    mgr, params, s, tr, mi, rays, _ = light_scene
    K = 3
    ta, *_ = loaded_tracer(rtx, mgr, 0)
    with ta:
        ta.render(0, 2 * K)
        want = ta.read_accum()
    tb, *_ = loaded_tracer(rtx, mgr, 0)
    with tb:
        tb.render(0, K)
        tb.render_aov(0, 2)
        tb.denoise(iterations=2)
        tb.temporal()

        def state():
            return {"accum": tb.read_accum(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1), "denoised": tb.read_denoised(),
                    "temporal": tb.read_temporal(), "history": tb.read_temporal_history(), "aov_info": tb.aov_info(),
                    "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(), "stats": tb.stats()}
        before = state()
        tb.trace_radiance(rays[:500], 16, seed=1)
        tb.trace_radiance(far_rays(rtx, tr, 64, 1e4, seed=2), 4)       # widens the padding
        tb.trace_radiance(rays[:10])                                  # the defaults
        after = state()
        for k in ("accum", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        tb.render(K, K)
        assert tb.read_accum().tobytes() == want.tobytes()


def test_error_codes_defaults_and_info(rtx, light_scene):
    mgr, params, s, tr, mi, rays, _ = light_scene
    lib = rtx.load_library()
    r = np.ascontiguousarray(rays[:8])
    out = np.full((8, 4), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def q(samples=4, seed=0, first=0, reserved=None):
        a = np.zeros((), rtx.RADIANCE_PARAMS)
        a["samples"], a["seed"], a["firstIndex"] = samples, seed, first
        if reserved is not None:
            a["_reserved"][reserved] = 1
        return a
    ok = q()
    assert lib.rt_trace_radiance(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_trace_radiance_device(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_multi_trace_radiance(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_get_radiance_info(None, None) == -1
    with rtx.Tracer(0) as t:
        c = t._ctx
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        for call in (lib.rt_trace_radiance, lib.rt_trace_radiance_device):
            assert call(c, p(r), 8, p(ok), p(out)) == -2 and b"rt_set_params" in lib.rt_last_error(c)      # no params set
        t.set_params(params)
        for call in (lib.rt_trace_radiance, lib.rt_trace_radiance_device):
            assert call(c, p(r), 0, p(ok), None) == 0 and call(c, None, 0, None, None) == 0
            assert call(c, p(r), -1, p(ok), p(out)) == -2
            assert call(c, None, 8, p(ok), p(out)) == -2 and call(c, p(r), 8, p(ok), None) == -2
            for bad in (q(0), q(-1), q(65537), q(reserved=0), q(reserved=4)):
                assert call(c, p(r), 8, p(bad), p(out)) == -2, bad
                assert lib.rt_last_error(c)
        assert lib.rt_trace_radiance_device(c, p(r), 8, p(ok), p(out)) == -2 and b"device" in lib.rt_last_error(c)      # host memory
        assert (out == 7.0).all()
        info = t.radiance_info()
        assert info["calls"] == 0 and info["lastKernelMs"] == 0 and info["totalKernelMs"] == 0, info
        assert lib.rt_trace_radiance(c, p(r), 8, p(q(65536)), p(out)) == 0 and (out[:, 3] == 1).all()           # the largest N is legal
        # params == NULL: the context's numRaysPerPixel samples, seed 0, firstIndex 0
        n = int(params["numRaysPerPixel"])
        rc.assert_same_bits(t.trace_radiance(rays[:300]), t.trace_radiance(rays[:300], n, 0, 0), "defaults")
        info = t.radiance_info()
        assert info["calls"] == 3 and info["samples"] == n and info["lastKernelMs"] > 0 and info["totalKernelMs"] > info["lastKernelMs"], info
    with rtx.MultiTracer([0] * 2) as m:
        assert lib.rt_multi_trace_radiance(m._m, p(r), 8, p(ok), p(out)) == -2      # no params set
        m.set_params(params)
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        assert lib.rt_multi_trace_radiance(m._m, p(r), 0, None, None) == 0
        assert lib.rt_multi_trace_radiance(m._m, p(r), -1, p(ok), p(out)) == -2 and lib.rt_multi_trace_radiance(m._m, None, 8, p(ok), p(out)) == -2
        assert lib.rt_multi_trace_radiance(m._m, p(r), 8, p(q(0)), p(out)) == -2
        assert lib.rt_multi_last_error(m._m)


def test_manager_method(rtx, light_scene):
    _, params, s, tr, mi, rays, want = light_scene
    mgr = light_manager(rtx)
    with rtx.Tracer(0) as t:
        mgr.backend = t
        got = mgr.TraceRadiance(rays[:200], 16, seed=7, firstIndex=11)
    rc.assert_same_bits(got, want(16, int(params["maxBounceCount"]))[:200], "RayTracingManager.TraceRadiance")
