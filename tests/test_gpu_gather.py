"""Gather queries on the GPU (rt_gather and its device and rt_multi forms): every float of every result bitwise against the checker
(tests/query_oracle.c: the oracle's own random_direction() and trace() per point and sample) and, with no checker in between, against
the radiance kernel; invisible slicing, rt_multi, a spilling traversal stack, far origins, special values, the device entry; a call
leaves every other state of the context alone.  The points are the first hits of a scene's 64 x 48 camera rays (rt_trace_rays):
hitPoint + 1e-3 * normal with the normal, misses kept with n = 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import query_check as gc
from ray_query_helpers import camera_rays, make_rays, scene_of
from test_gpu_radiance import light_manager
from test_gpu_ray_query import far_rays, loaded_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (gc.COSINE, gc.SH9)
SEED, FIRST = 7, 11


def points_of(rtx, tracer, params):
    pts = gc.surface_points(rtx, tracer.trace_rays(camera_rays(rtx, params)))
    assert (pts["direction"] != 0).any(1).sum() > len(pts) // 2           # mostly hits
    return pts


def check(rtx, tracer, params, spheres, tris, infos, pts, samples, mode, what, seed=0, first_index=0):
    """pts on `tracer` (which holds the scene and params) against the checker; returns the result"""
    want = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, samples, seed, first_index, mode)
    got = tracer.gather(pts, samples, seed, first_index, mode)
    gc.assert_same_bits(got, want, what)
    return got


@pytest.fixture(scope="module")
def light_scene(rtx):
    """the scene most tests share, its points, and the checker's answers by (samples, maxBounceCount, mode), computed once"""
    mgr = light_manager(rtx)
    params, spheres, tris, infos = mgr.build_buffers()
    assert (infos["material"]["flag"] == 2).any()
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        pts = points_of(rtx, t, params)
    pts.setflags(write=False)
    cache = {}

    def want(samples, bounces, mode):
        if (samples, bounces, mode) not in cache:
            p = params.copy()
            p["maxBounceCount"] = bounces
            cache[samples, bounces, mode] = gc.oracle_gather(rtx, p, spheres, tris, infos, pts, samples, SEED, FIRST, mode)
            cache[samples, bounces, mode].setflags(write=False)
        return cache[samples, bounces, mode]
    return mgr, params, spheres, tris, infos, pts, want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("name", ["light", "Reflective_Balls"])
def test_surface_points_of_the_scenes(rtx, name, intersect, mode):
    """spheres, triangles, a checker floor and emitting InvisibleLights (pass-through casts on sample 0 and on later samples), in
    FLAT_CHUNKS and BVH mode; Reflective_Balls is the scene that caught a bool carried across the traversal"""
    mgr = light_manager(rtx) if name == "light" else scene_of(rtx, name)
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, intersect)
    assert len(s) > 0 and len(tr) > 0
    with t:
        pts = points_of(rtx, t, params)
        got = check(rtx, t, params, s, tr, mi, pts, 21, mode, f"{name} intersect {intersect} mode {mode}", seed=1)
        flat = got.reshape(len(pts), -1)
        assert (flat[:, 3] == 1).all() and len(np.unique(flat[:, :3], axis=0)) > 16
        info = t.gather_info()
        assert info["lastSampleLanes"] == 16 and info["mode"] == mode and info["samples"] == 21


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("samples", [1, 3, 4, 16, 64])
def test_sample_counts_and_batch_sizes(rtx, light_scene, samples, mode):
    """n = 1 and 5 leave most lanes of a wave without a point, 67 ends inside a wave, 3072 spans blocks"""
    mgr, params, s, tr, mi, pts, want = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        full = want(samples, int(params["maxBounceCount"]), mode)
        for n in (1, 5, 67, 3072):
            # (a batch of the first n points has the stream indices of the whole batch's first n)
            got = t.gather(pts[:n], samples, SEED, FIRST, mode)
            gc.assert_same_bits(got, full[:n], f"samples {samples}, n {n}, mode {mode}")
        info = t.gather_info()
        assert info["lastSampleLanes"] == (16 if samples >= 16 else 4 if samples >= 4 else 1)
        assert info["samples"] == samples and info["mode"] == mode


@pytest.mark.parametrize("bounces", [0, 1, 8])
@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_node_forms_builders_and_bounce_limits(rtx, light_scene, compact_nodes, device_bvh, bounces):
    mgr, params, s, tr, mi, pts, want = light_scene
    p = params.copy()
    p["maxBounceCount"] = bounces
    with rtx.Tracer(0) as t:
        t.set_option("compact_nodes", compact_nodes)
        t.set_option("device_bvh", device_bvh)
        t.set_params(p)
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        for mode in MODES:
            got = t.gather(pts, 16, SEED, FIRST, mode)
            gc.assert_same_bits(got, want(16, bounces, mode), f"compact_nodes {compact_nodes} device_bvh {device_bvh} bounces {bounces} mode {mode}")


def test_one_sample_is_the_radiance_kernel_along_the_drawn_direction(rtx, light_scene):
    """k_gather against k_radiance, no checker in between: N = 1, mode 0 == rt_trace_radiance with samples 1, the same seed and
    firstIndex, over the rays (origin, the sample's direction, tMax)"""
    mgr, params, s, tr, mi, pts, _ = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        p = pts[:1024].copy()
        p["tMax"][1::3] = np.float32(2.5)                                # a bound that rejects some first hits
        p["tMax"][2::17] = 0.0
        d = gc.directions(rtx, p, 0, SEED, 0xFFFFFE00, gc.COSINE)        # (the index wraps inside the batch)
        rays = make_rays(rtx, p["origin"], d, p["tMax"])
        got = t.gather(p, 1, SEED, 0xFFFFFE00, gc.COSINE)
        gc.assert_same_bits(got, t.trace_radiance(rays, 1, SEED, 0xFFFFFE00), "gather N = 1 against the radiance query")
        assert (got[2::17] == 0).all() and len(np.unique(got[:, :3], axis=0)) > 16


@pytest.mark.parametrize("mode", MODES)
def test_slices_and_split_calls_are_invisible(rtx, light_scene, mode):
    mgr, params, s, tr, mi, pts, want = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        r = pts[:1000]
        whole = t.gather(r, 5, SEED, FIRST, mode)
        gc.assert_same_bits(whole, want(5, int(params["maxBounceCount"]), mode)[:1000], "default slice")
        for slice_ in (1, 7, 1000):
            t.set_option("gather_slice", slice_)
            gc.assert_same_bits(t.gather(r, 5, SEED, FIRST, mode), whole, f"gather_slice {slice_}")
        t.set_option("gather_slice", 1 << 20)
        a = t.gather(r[:377], 5, SEED, FIRST, mode)
        b = t.gather(r[377:], 5, SEED, FIRST + 377, mode)
        gc.assert_same_bits(np.concatenate([a, b]), whole, "two calls")
        # firstIndex wraps inside the batch
        wrap = check(rtx, t, params, s, tr, mi, r[:512], 4, mode, "firstIndex 0xFFFFFF00", seed=2, first_index=0xFFFFFF00)
        t.set_option("gather_slice", 100)
        gc.assert_same_bits(t.gather(r[:512], 4, 2, 0xFFFFFF00, mode), wrap, "firstIndex 0xFFFFFF00, gather_slice 100")


@pytest.mark.parametrize("contexts", [2, 3])
def test_multi_tracer_gives_the_single_context_bits(rtx, light_scene, contexts):
    mgr, params, s, tr, mi, pts, want = light_scene
    with rtx.MultiTracer([0] * contexts) as m:
        m.set_params(params)
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        for mode in MODES:
            got = m.gather(pts[:2999], 16, SEED, FIRST, mode)
            gc.assert_same_bits(got, want(16, int(params["maxBounceCount"]), mode)[:2999], f"{contexts} contexts, mode {mode}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, compact_nodes):
    """three stack entries per lane in LDS, the rest of the Knight's tree in the global overflow area (both node forms)"""
    mgr = scene_of(rtx, "Knight")
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes)
    with t:
        pts = gc.surface_points(rtx, t.trace_rays(camera_rays(rtx, params, 48, 32)))
        got = {mode: check(rtx, t, params, s, tr, mi, pts, 16, mode, f"lds_stack 3 compact_nodes {compact_nodes} mode {mode}") for mode in MODES}
        assert t.stats()["bvhMaxStack"] > 3         # (the overflow area was in use)
    t, *_ = loaded_tracer(rtx, mgr, 0, compact_nodes=compact_nodes)
    with t:
        for mode in MODES:
            gc.assert_same_bits(t.gather(pts, 16, mode=mode), got[mode], "against the whole stack in LDS")


def test_far_origins_widen_the_padding(rtx, light_scene):
    mgr, params, s, tr, mi, pts, _ = light_scene
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        check(rtx, t, params, s, tr, mi, pts[:256], 4, gc.COSINE, "near")
        repads = t.stats()["bvhRepads"]
        far = far_rays(rtx, tr, 512, 1e5, seed=9)                       # the "normal" points at the scene, not normalised: used as given
        far["direction"] /= np.linalg.norm(far["direction"], axis=1, keepdims=True)
        far["direction"][::2] = 0.0                                     # the whole sphere for half of them
        got = check(rtx, t, params, s, tr, mi, far, 4, gc.COSINE, "origins 1e5 away")
        assert t.stats()["bvhRepads"] > repads
        assert len(np.unique(got[:, :3], axis=0)) > 16
        check(rtx, t, params, s, tr, mi, far, 4, gc.SH9, "origins 1e5 away, SH9")


@pytest.mark.parametrize("mode", MODES)
def test_bounds_and_special_values(rtx, light_scene, mode):
    mgr, *_ = light_scene
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 1)
    with t:
        pts = points_of(rtx, t, params)[:1536].copy()
        pts["tMax"][1::4] = np.float32(2.5)                             # a finite bound: some first hits lie beyond it
        pts["tMax"][2::16] = np.float32(0.0)
        pts["tMax"][6::16] = np.float32(np.nan)
        pts["tMax"][10::16] = np.float32(-1.0)
        got = check(rtx, t, params, s, tr, mi, pts, 5, mode, f"mixed tMax mode {mode}", seed=2, first_index=0xFFFFFF00)
        flat = got.reshape(len(pts), -1)
        assert (flat[2::16] == 0).all() and (flat[6::16] == 0).all() and (flat[10::16] == 0).all() and (flat[:, 3] == 1).any()
        unbounded = pts.copy()
        unbounded["tMax"] = np.inf
        free = t.gather(unbounded, 5, 2, 0xFFFFFF00, mode)
        assert (free[1::4] != got[1::4]).any()                          # (the bound changed some answers)
        # NaN / inf / zero / unnormalised normals and NaN / inf origins: whatever the arithmetic gives, the checker's bits
        o, n = np.asarray(pts["origin"][:64]).copy(), np.asarray(pts["direction"][:64]).copy()
        o[:8, 0], o[8:16, 1], o[16:24, 2] = np.nan, np.inf, -np.inf
        n[24:32, 0], n[32:40, 1], n[40:48], n[48:56] = np.nan, np.inf, 0.0, n[48:56] * np.float32(3.0)
        check(rtx, t, params, s, tr, mi, make_rays(rtx, o, n), 4, mode, f"NaN / inf / zero mode {mode}")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/gather_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "gather_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gather device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


STATS_MAY_MOVE = ("bvhBuilds", "bvhRebuilds", "bvhRepads")


def test_a_call_moves_no_other_state(rtx, light_scene):
    mgr, params, s, tr, mi, pts, _ = light_scene
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
        tb.trace_radiance(camera_rays(rtx, params)[:100], 4)

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "stats": tb.stats()}
        before = state()
        far = far_rays(rtx, tr, 64, 1e4, seed=2)
        tb.gather(pts[:500], 16, seed=1)
        tb.gather(pts[:500], 16, seed=1, mode=gc.SH9)
        tb.gather(far, 4)                                              # widens the padding
        tb.gather(pts[:10])                                            # the defaults
        after = state()

        def same(before, after):
            for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
                assert before[k].tobytes() == after[k].tobytes(), k
            for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info"):
                assert before[k] == after[k], k
            for k, v in before["stats"].items():
                if k not in STATS_MAY_MOVE:
                    assert np.array_equal(v, after["stats"][k]), k
        same(before, after)
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            tb.gather(pts[:64], 4, mode=f % 2)
        assert tb.read_accum().tobytes() == want.tobytes()


def test_error_codes_defaults_and_info(rtx, light_scene):
    mgr, params, s, tr, mi, pts, _ = light_scene
    lib = rtx.load_library()
    r = np.ascontiguousarray(pts[:8])
    out = np.full(8 * 36, 7.0, np.float32)                   # room for either mode
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def q(samples=4, seed=0, first=0, mode=0, reserved=None):
        a = np.zeros((), rtx.GATHER_PARAMS)
        a["samples"], a["seed"], a["firstIndex"], a["mode"] = samples, seed, first, mode
        if reserved is not None:
            a["_reserved"][reserved] = 1
        return a
    ok = q()
    assert lib.rt_gather(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_gather_device(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_multi_gather(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_get_gather_info(None, None) == -1
    with rtx.Tracer(0) as t:
        c = t._ctx
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        for call in (lib.rt_gather, lib.rt_gather_device):
            assert call(c, p(r), 8, p(ok), p(out)) == -2 and b"rt_set_params" in lib.rt_last_error(c)      # no params set
        t.set_params(params)
        stats = t.stats()
        for call in (lib.rt_gather, lib.rt_gather_device):
            assert call(c, p(r), 0, p(ok), None) == 0 and call(c, None, 0, None, None) == 0
            assert call(c, p(r), -1, p(ok), p(out)) == -2
            assert call(c, None, 8, p(ok), p(out)) == -2 and call(c, p(r), 8, p(ok), None) == -2
            for bad in (q(0), q(-1), q(65537), q(reserved=0), q(reserved=3), q(mode=2), q(mode=-1)):
                assert call(c, p(r), 8, p(bad), p(out)) == -2, bad
                assert lib.rt_last_error(c)
        assert lib.rt_gather_device(c, p(r), 8, p(ok), p(out)) == -2 and b"device" in lib.rt_last_error(c)      # host memory
        assert (out == 7.0).all()
        info = t.gather_info()
        assert info["calls"] == 0 and info["lastKernelMs"] == 0 and info["totalKernelMs"] == 0 and info["samples"] == 0, info
        assert all(np.array_equal(v, t.stats()[k]) for k, v in stats.items())
        assert lib.rt_gather(c, p(r), 8, p(q(65536)), p(out)) == 0 and (out[:32].reshape(8, 4)[:, 3] == 1).all() and (out[32:] == 7.0).all()      # the largest N is legal; mode 0 writes n * 4 floats
        # params == NULL: the context's numRaysPerPixel samples, seed 0, firstIndex 0, mode 0
        n = int(params["numRaysPerPixel"])
        gc.assert_same_bits(t.gather(pts[:300]), t.gather(pts[:300], n, 0, 0, 0), "defaults")
        info = t.gather_info()
        assert info["calls"] == 3 and info["samples"] == n and info["mode"] == 0, info
        assert info["lastKernelMs"] > 0 and info["totalKernelMs"] > info["lastKernelMs"], info
    with rtx.MultiTracer([0] * 2) as m:
        assert lib.rt_multi_gather(m._m, p(r), 8, p(ok), p(out)) == -2      # no params set
        m.set_params(params)
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        assert lib.rt_multi_gather(m._m, p(r), 0, None, None) == 0
        assert lib.rt_multi_gather(m._m, p(r), -1, p(ok), p(out)) == -2 and lib.rt_multi_gather(m._m, None, 8, p(ok), p(out)) == -2
        assert lib.rt_multi_gather(m._m, p(r), 8, p(q(0)), p(out)) == -2 and lib.rt_multi_gather(m._m, p(r), 8, p(q(mode=2)), p(out)) == -2
        assert lib.rt_multi_last_error(m._m)


def test_manager_method(rtx, light_scene):
    _, params, s, tr, mi, pts, want = light_scene
    mgr = light_manager(rtx)
    with rtx.Tracer(0) as t:
        mgr.backend = t
        for mode in MODES:
            got = mgr.Gather(pts[:200], 16, seed=SEED, firstIndex=FIRST, mode=mode)
            gc.assert_same_bits(got, want(16, int(params["maxBounceCount"]), mode)[:200], f"RayTracingManager.Gather mode {mode}")
