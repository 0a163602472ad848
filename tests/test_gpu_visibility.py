"""Visibility gathers on the GPU (rt_visibility and its device and rt_multi forms): every float of every result bitwise against the checker
(tests/query_oracle.c: the oracle's own random_direction() and calculate_ray_collision() per point and sample) and, with no checker
in between, against rt_occluded and rt_trace_rays over the same rays; invisible slicing, rt_multi, a spilling traversal stack, the
device entry; a call needs no rt_params and leaves every other state of the context alone.

The batch is 65 points: the first hits of 61 camera rays of the mixed scene (hitPoint + 1e-3 * normal with the normal, misses kept with
n = 0), a point with n = 0 and three points that are not traced (t = 0, -1, NaN) near its start, so that every prefix the tests take
(1, 3, 5, 17, 65 points: with S = 16, 4 and 1 lanes per point 5, 17 and 65 points end inside a wave) holds some of them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import query_check as vc
from ray_query_helpers import camera_rays, scene_of
from test_gpu_radiance import light_manager
from test_gpu_ray_query import far_rays, loaded_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = [1, 3, 4, 5, 16, 17, 21, 64]
SIZES = [1, 3, 5, 17, 65]
SEED, FIRST = 7, 0xFFFFFFE0                                               # (the index wraps inside the batch)
SCENES = ("mixed", "spheres", "triangles")


def buffers_of(rtx, which):
    """the light scene whole, its spheres alone, its triangles alone"""
    params, s, tr, mi = light_manager(rtx).build_buffers()
    if which == "spheres":
        tr, mi = tr[:0], mi[:0]
    elif which == "triangles":
        s = s[:0]
    return params, s, tr, mi


def tracer_of(rtx, which, intersect=0, **options):
    params, s, tr, mi = buffers_of(rtx, which)
    params["intersectMode"] = intersect
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=s, triangles=tr, meshinfo=mi)
    return t


@pytest.fixture(scope="module")
def batch(rtx):
    """the 65 points and the checker's answers by (scene, intersect, mode, samples), each computed once"""
    params, s, tr, mi = buffers_of(rtx, "mixed")
    with tracer_of(rtx, "mixed") as t:
        hits = t.trace_rays(camera_rays(rtx, params)[11::50][:61])
    assert len(hits) == 61 and len(s) > 0 and len(tr) > 0
    got = vc.surface_points(rtx, hits)
    assert (got["direction"] != 0).any(1).sum() > 30
    pts = np.zeros(65, rtx.RAY)
    special = [1, 2, 3, 9]
    pts[[i for i in range(65) if i not in special]] = got
    pts["tMax"][4::6] = np.float32(2.5)                                   # a finite reach: some hits lie beyond it
    pts[1], pts[3], pts[9] = got[0], got[1], got[2]
    pts["tMax"][1], pts["tMax"][3], pts["tMax"][9] = 0.0, -1.0, np.nan    # not traced
    pts[2] = got[0]
    pts["direction"][2] = 0.0                                             # n = 0: the whole sphere
    pts.setflags(write=False)
    cache = {}

    def want(which, intersect, mode, samples):
        key = (which, intersect, mode, samples)
        if key not in cache:
            _, ss, tt, mm = buffers_of(rtx, which)
            cache[key] = vc.oracle_visibility(rtx, ss, tt, mm, pts, samples, SEED, FIRST, mode, intersect)
            cache[key].setflags(write=False)
        return cache[key]
    return pts, want


def zero_rows(got):
    return (got[[1, 3, 9]].view(np.uint32) == 0).all()


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("which", SCENES)
def test_scenes_modes_node_forms_builders_and_sample_counts(rtx, batch, which, intersect, compact_nodes, device_bvh):
    pts, want = batch
    with tracer_of(rtx, which, intersect, compact_nodes=compact_nodes, device_bvh=device_bvh) as t:
        for mode in vc.MODES:
            for samples in COUNTS:
                got = t.visibility(pts, samples, SEED, FIRST, mode)
                vc.assert_same_bits(got, want(which, intersect, mode, samples),
                                    f"{which} intersect {intersect} compact_nodes {compact_nodes} device_bvh {device_bvh} mode {mode} samples {samples}")
                assert zero_rows(got)
                info = t.visibility_info()
                assert info["lastSampleLanes"] == (16 if samples >= 16 else 4 if samples >= 4 else 1)
                assert info["samples"] == samples and info["mode"] == mode
        cos = want(which, intersect, vc.COSINE, 64)
        assert 0 < (cos[:, 3] == 1).sum() and len(np.unique(cos[:, 3])) > 4          # open points, and every degree of occlusion


@pytest.mark.parametrize("mode", vc.MODES)
def test_batch_sizes_leave_partial_waves(rtx, batch, mode):
    """a batch of the first n points has the stream indices of the whole batch's first n"""
    pts, want = batch
    with tracer_of(rtx, "mixed") as t:
        for samples in COUNTS:
            full = want("mixed", 0, mode, samples)
            for n in SIZES:
                vc.assert_same_bits(t.visibility(pts[:n], samples, SEED, FIRST, mode), full[:n], f"samples {samples}, n {n}, mode {mode}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, compact_nodes):
    """three stack entries per lane in LDS, the rest of the Knight's tree in the global overflow area (both node forms)"""
    mgr = scene_of(rtx, "Knight")
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes)
    with t:
        pts = vc.surface_points(rtx, t.trace_rays(camera_rays(rtx, params, 48, 32)[5::24]))
        assert len(pts) == 64 and (pts["direction"] != 0).any(1).sum() > 8
        got = {}
        for mode in vc.MODES:
            got[mode] = t.visibility(pts, 16, 3, 5, mode)
            vc.assert_same_bits(got[mode], vc.oracle_visibility(rtx, s, tr, mi, pts, 16, 3, 5, mode, 0), f"lds_stack 3 compact_nodes {compact_nodes} mode {mode}")
        assert t.stats()["bvhMaxStack"] > 3         # (the overflow area was in use)
    t, *_ = loaded_tracer(rtx, mgr, 0, compact_nodes=compact_nodes)
    with t:
        for mode in vc.MODES:
            vc.assert_same_bits(t.visibility(pts, 16, 3, 5, mode), got[mode], "against the whole stack in LDS")


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("samples", [5, 21])
def test_the_existing_kernels_give_the_same_answers_ray_by_ray(rtx, batch, samples, intersect):
    """k_visibility against k_ray_query, no checker's cast in between: the test makes the n x N rays (origin, the checker's direction,
    reach) itself.  Every point and every sample of the batch."""
    pts, _ = batch
    n, N = len(pts), samples
    with tracer_of(rtx, "mixed", intersect) as t:
        for mode in (vc.COSINE, vc.SH9):
            rays = vc.sample_rays(rtx, pts, N, SEED, FIRST, mode)
            occluded = np.asarray(t.occluded(rays)).reshape(n, N).astype(np.int64)
            got = t.visibility(pts, N, SEED, FIRST, mode)
            vis = got[:, 3] if mode == vc.COSINE else got[:, 9]
            traced = pts["tMax"] > 0
            open_ = (N - occluded.sum(1))[traced]
            # visibility x N is the open count: the quotient count / (float)N is exact to the bit (distinct counts give distinct quotients),
            # and the product rounds back to the count (in float32 (17 / 21) * 21 is not 17 to the last bit, so the product is rounded)
            assert (vis[traced] == open_.astype(np.float32) / np.float32(N)).all(), f"mode {mode}"
            assert (np.rint(vis[traced].astype(np.float64) * N) == open_).all(), f"mode {mode}"
            assert (occluded[~traced] == 0).all() and (vis[~traced] == 0).all()
            assert 0 < occluded.sum() < traced.sum() * N
        rays = vc.sample_rays(rtx, pts, N, SEED, FIRST, vc.DISTANCE)
        hits = t.trace_rays(rays).reshape(n, N)
        got = t.visibility(pts, N, SEED, FIRST, vc.DISTANCE)
        for i in range(n):
            if not pts["tMax"][i] > 0:
                assert (got[i].view(np.uint32) == 0).all()
                continue
            hit = hits["kind"][i] != 0
            r = np.where(hit, hits["dst"][i], pts["tMax"][i]).astype(np.float32)
            with np.errstate(all="ignore"):
                ch = np.stack([r, r * r, hit.astype(np.float32)], 1)
                vc.assert_same_bits(got[i], vc.finish(vc.tree_sum(ch), vc.DISTANCE), f"distance, point {i}")


@pytest.mark.parametrize("mode", vc.MODES)
def test_slices_and_split_calls_are_invisible(rtx, batch, mode):
    pts, want = batch
    with tracer_of(rtx, "mixed") as t:
        r = pts[:20]
        whole = t.visibility(r, 5, SEED, FIRST, mode)
        vc.assert_same_bits(whole, want("mixed", 0, mode, 5)[:20], "default slice")
        for slice_ in (1, 7, 20):
            t.set_option("visibility_slice", slice_)
            vc.assert_same_bits(t.visibility(r, 5, SEED, FIRST, mode), whole, f"visibility_slice {slice_}")
        t.set_option("visibility_slice", 1 << 22)
        for cut in (1, 7, 19):
            a = t.visibility(r[:cut], 5, SEED, FIRST, mode)
            b = t.visibility(r[cut:], 5, SEED, FIRST + cut, mode)
            vc.assert_same_bits(np.concatenate([a, b]), whole, f"two calls, cut at {cut}")
        assert (t.visibility(r, 5, SEED, 0, mode) != whole).any() and (t.visibility(r, 5, SEED + 1, FIRST, mode) != whole).any()


@pytest.mark.parametrize("contexts", [2, 3])
def test_multi_tracer_gives_the_single_context_bits(rtx, batch, contexts):
    pts, want = batch
    params, s, tr, mi = buffers_of(rtx, "mixed")
    with rtx.MultiTracer([0] * contexts) as m:
        m.upload(spheres=s, triangles=tr, meshinfo=mi)                    # (no params: the call needs none)
        for mode in vc.MODES:
            vc.assert_same_bits(m.visibility(pts, 16, SEED, FIRST, mode), want("mixed", 0, mode, 16), f"{contexts} contexts, mode {mode}")
            vc.assert_same_bits(m.visibility(pts[:2], 4, SEED, FIRST, mode), want("mixed", 0, mode, 4)[:2], "fewer points than contexts")


def test_far_origins_widen_the_padding(rtx, batch):
    pts, _ = batch
    params, s, tr, mi = buffers_of(rtx, "mixed")
    with tracer_of(rtx, "mixed") as t:
        t.visibility(pts, 4)
        repads = t.stats()["bvhRepads"]
        far = far_rays(rtx, tr, 64, 1e5, seed=9)                          # the "normal" points at the scene, not normalised: used as given
        far["direction"][::2] = 0.0
        for mode in vc.MODES:
            vc.assert_same_bits(t.visibility(far, 4, 1, 2, mode), vc.oracle_visibility(rtx, s, tr, mi, far, 4, 1, 2, mode), f"origins 1e5 away, mode {mode}")
        assert t.stats()["bvhRepads"] > repads


@pytest.mark.parametrize("mode", vc.MODES)
def test_special_values(rtx, batch, mode):
    """NaN / inf / zero / unnormalised normals and NaN / inf origins: whatever the arithmetic gives, the checker's bits"""
    pts, _ = batch
    params, s, tr, mi = buffers_of(rtx, "mixed")
    keep = [i for i in range(65) if i not in (1, 3, 9)][:56]
    o, n = np.asarray(pts["origin"][keep]).copy(), np.asarray(pts["direction"][keep]).copy()
    o[:8, 0], o[8:16, 1], o[16:24, 2] = np.nan, np.inf, -np.inf
    n[24:32, 0], n[32:40, 1], n[40:48], n[48:56] = np.nan, np.inf, 0.0, n[48:56] * np.float32(3.0)
    special = np.zeros(56, rtx.RAY)
    special["origin"], special["direction"], special["tMax"] = o, n, np.inf
    special["tMax"][::5] = 2.5
    with tracer_of(rtx, "mixed", 1) as t:
        vc.assert_same_bits(t.visibility(special, 5, 2, 3, mode), vc.oracle_visibility(rtx, s, tr, mi, special, 5, 2, 3, mode, 1), f"mode {mode}")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/visibility_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "visibility_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "visibility device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


STATS_MAY_MOVE = ("bvhBuilds", "bvhRebuilds", "bvhRepads")


def test_a_context_without_params_answers(rtx, batch):
    pts, want = batch
    params, s, tr, mi = buffers_of(rtx, "mixed")
    with rtx.Tracer(0) as t:
        t.upload(spheres=s, triangles=tr, meshinfo=mi)                    # never rt_set_params: intersectMode is RT_INTERSECT_FLAT_CHUNKS
        for mode in vc.MODES:
            vc.assert_same_bits(t.visibility(pts, 16, SEED, FIRST, mode), want("mixed", 0, mode, 16), f"no params, mode {mode}")
        # params == NULL: 64 samples, seed 0, firstIndex 0, mode 0
        vc.assert_same_bits(t.visibility(pts), t.visibility(pts, 64, 0, 0, 0), "defaults")
        info = t.visibility_info()
        assert info["calls"] == 5 and info["samples"] == 64 and info["mode"] == 0 and info["lastSampleLanes"] == 16, info
        assert info["lastKernelMs"] > 0 and info["totalKernelMs"] > info["lastKernelMs"], info


def test_a_call_moves_no_other_state(rtx, batch):
    pts, _ = batch
    mgr = light_manager(rtx)
    params, s, tr, mi = mgr.build_buffers()
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
        tb.gather(pts, 4)

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "gather_info": tb.gather_info(), "stats": tb.stats()}
        before = state()
        assert tb.visibility_info()["calls"] == 0
        for k, (mode, samples) in enumerate(((vc.COSINE, 16), (vc.SH9, 5), (vc.DISTANCE, 1))):
            tb.visibility(pts, samples, seed=1, mode=mode)
            info = tb.visibility_info()
            assert (info["calls"], info["mode"], info["samples"], info["lastSampleLanes"]) == (k + 1, mode, samples, (16, 4, 1)[k]), info
        tb.visibility(far_rays(rtx, tr, 64, 1e4, seed=2), 4)              # widens the padding
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            tb.visibility(pts, 4, mode=f % 3)
        assert tb.read_accum().tobytes() == want.tobytes()


def test_error_codes_leave_everything_untouched(rtx, batch):
    pts, _ = batch
    params, s, tr, mi = buffers_of(rtx, "mixed")
    lib = rtx.load_library()
    r = np.ascontiguousarray(pts[:8])
    out = np.full(8 * 12, 7.0, np.float32)                   # room for every mode
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def q(samples=4, seed=0, first=0, mode=0, reserved=None):
        a = np.zeros((), rtx.VISIBILITY_PARAMS)
        a["samples"], a["seed"], a["firstIndex"], a["mode"] = samples, seed, first, mode
        if reserved is not None:
            a["_reserved"][reserved] = 1
        return a
    ok = q()
    assert lib.rt_visibility(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_visibility_device(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_multi_visibility(None, p(r), 8, p(ok), p(out)) == -1
    assert lib.rt_get_visibility_info(None, None) == -1
    with rtx.Tracer(0) as t:
        c = t._ctx
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        stats = t.stats()
        for call in (lib.rt_visibility, lib.rt_visibility_device):
            assert call(c, p(r), 0, p(ok), None) == 0 and call(c, None, 0, None, None) == 0
            assert call(c, p(r), -1, p(ok), p(out)) == -2
            assert call(c, None, 8, p(ok), p(out)) == -2 and call(c, p(r), 8, p(ok), None) == -2
            for bad in (q(0), q(-1), q(65537), q(reserved=0), q(reserved=3), q(mode=3), q(mode=-1)):
                assert call(c, p(r), 8, p(bad), p(out)) == -2, bad
                assert lib.rt_last_error(c)
        assert lib.rt_visibility_device(c, p(r), 8, p(ok), p(out)) == -2 and b"device" in lib.rt_last_error(c)      # host memory
        assert (out == 7.0).all()
        info = t.visibility_info()
        assert info["calls"] == 0 and info["lastKernelMs"] == 0 and info["totalKernelMs"] == 0 and info["samples"] == 0, info
        assert all(np.array_equal(v, t.stats()[k]) for k, v in stats.items())
        assert lib.rt_visibility(c, p(r), 8, p(q(65536, mode=2)), p(out)) == 0       # the largest N is legal; modes 0 and 2 write n * 4 floats
        assert (out[:32].reshape(8, 4)[[0, 2, 4, 5, 6, 7], 3] == 1).all() and (out[32:] == 7.0).all()
        assert t.visibility_info()["calls"] == 1
    with rtx.MultiTracer([0] * 2) as m:
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        assert lib.rt_multi_visibility(m._m, p(r), 0, None, None) == 0
        assert lib.rt_multi_visibility(m._m, p(r), -1, p(ok), p(out)) == -2 and lib.rt_multi_visibility(m._m, None, 8, p(ok), p(out)) == -2
        assert lib.rt_multi_visibility(m._m, p(r), 8, p(q(0)), p(out)) == -2 and lib.rt_multi_visibility(m._m, p(r), 8, p(q(mode=3)), p(out)) == -2
        assert lib.rt_multi_visibility(m._m, p(r), 8, p(q(reserved=1)), p(out)) == -2
        assert lib.rt_multi_last_error(m._m)


def test_manager_method(rtx, batch):
    pts, want = batch
    mgr = light_manager(rtx)
    with rtx.Tracer(0) as t:
        mgr.backend = t
        for mode in vc.MODES:
            vc.assert_same_bits(mgr.Visibility(pts, 16, seed=SEED, firstIndex=FIRST, mode=mode), want("mixed", 0, mode, 16), f"RayTracingManager.Visibility mode {mode}")
