"""Closest-point queries on the GPU (rt_closest_points and its device and rt_multi forms): every field of every record bit for bit
against the brute-force checker (tests/closest_oracle.c, pinned by tests/test_closest_cpu.py), over the smallest scenes that can still
go wrong, points that make ties and zero distances, points and scenes far from the origin (where an absolute-error mistake in the
culling would show), both node forms, both builders, every leaf size, a traversal stack that spills, a refitted local-mesh scene,
invisible slicing and rt_multi, the device entry; refusals; the state a call leaves alone; and that the traversal prunes.

Every scene's batch: a jittered 8 x 8 x 8 grid over the bounding box inflated 1.5 x, every vertex, edge midpoint and centroid of up to
40 triangles, 16 points 1e4 extents away, and three points that are not searched (R = 0, -1, NaN)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
from ray_query_helpers import scene_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("one", "two", "plane", "spheres", "mixed", "Knight", "Suzanne")


def plane(rtx, nx, ny, size=8.0):
    """2 x nx x ny triangles tessellating [0, size]^2 at z = 0, one chunk, normals +z"""
    xs, ys = np.linspace(0, size, nx + 1, dtype=np.float32), np.linspace(0, size, ny + 1, dtype=np.float32)
    t = np.zeros(2 * nx * ny, rtx.TRIANGLE)
    k = 0
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], 0), (xs[i + 1], ys[j], 0), (xs[i + 1], ys[j + 1], 0), (xs[i], ys[j + 1], 0)
            t["posA"][k], t["posB"][k], t["posC"][k] = a, b, c
            t["posA"][k + 1], t["posB"][k + 1], t["posC"][k + 1] = a, c, d
            k += 2
    t["normalA"] = t["normalB"] = t["normalC"] = (0, 0, 1)
    m = np.zeros(1, rtx.MESHINFO)
    m["numTriangles"] = len(t)
    m["boundsMin"], m["boundsMax"] = (0, 0, 0), (size, size, 0)
    return np.zeros(0, rtx.SPHERE), t, m


def buffers_of(rtx, name):
    """(spheres, triangles, meshinfo)"""
    if name in ("one", "two"):
        s, t, m = plane(rtx, 1, 1, 4.0)
        if name == "one":
            t, m = t[:1].copy(), m.copy()
            m["numTriangles"] = 1
        return s, t, m
    if name == "plane":
        return plane(rtx, 8, 8)
    if name == "spheres":
        _, s, t, m = scene_of(rtx, "Balls_Outdoors").build_buffers()
        return s, t[:0], m[:0]
    _, s, t, m = scene_of(rtx, "mesh_test_scene" if name == "mixed" else name).build_buffers()
    return s, t, m


def batch_of(rtx, s, t, m, seed=1):
    """the points of the module docstring for a scene, R = +inf (the three unsearched ones apart)"""
    rng = np.random.default_rng(seed)
    live = np.concatenate([np.arange(i["firstTriangleIndex"], i["firstTriangleIndex"] + i["numTriangles"]) for i in m]) if len(m) else np.zeros(0, int)
    corners = [np.asarray(t[k][live], np.float64).reshape(-1, 3) for k in ("posA", "posB", "posC")] if len(live) else []
    if len(s):
        c, r = np.asarray(s["position"], np.float64), np.asarray(s["radius"], np.float64)[:, None]
        corners += [c - r, c + r]
    allp = np.concatenate(corners)
    lo, hi = allp.min(0), allp.max(0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5) * 1.5
    g = (np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) + rng.random((512, 3))) / 8.0
    pts = [mid - half + g * 2 * half]
    if len(live):
        pick = live[rng.permutation(len(live))[:40]]
        A, B, C = (np.asarray(t[k][pick], np.float64) for k in ("posA", "posB", "posC"))
        pts += [A, B, C, (A + B) / 2, (A + C) / 2, (B + C) / 2, (A + B + C) / 3]
    d = rng.standard_normal((16, 3))
    pts.append(mid + d / np.linalg.norm(d, axis=1, keepdims=True) * 1e4 * np.linalg.norm(half))
    pts.append(np.repeat(mid[None], 3, 0))
    p = cc.points_of(rtx, np.concatenate(pts))
    p["tMax"][-3:] = (0.0, -1.0, np.nan)
    return p


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, points, the checker's answer), each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            p = batch_of(rtx, s, t, m)
            want = cc.oracle_closest(rtx, s, t, m, p)
            for a in (p, want):
                a.setflags(write=False)
            cache[name] = (s, t, m, p, want)
        return cache[name]
    return get


def tracer_of(rtx, s, t, m, **options):
    tr = rtx.Tracer(0)
    for k, v in options.items():
        tr.set_option(k, v)
    tr.upload(spheres=s, triangles=t, meshinfo=m)            # (no params: the call needs none)
    return tr


def check_batch(rtx, tr, s, t, m, p, want, what):
    got = tr.closest_points(p)
    cc.assert_same_records(rtx, got, want, what)
    assert (got["kind"][-3:] == 0).all() and np.isposinf(got["dst"][-3:]).all()
    # the radius at the checker's median distance: about half the points miss, and the kept ones keep their bits
    finite = want["dst"][np.isfinite(want["dst"])]
    q = p.copy()
    q["tMax"][:-3] = np.median(finite)
    wq = cc.oracle_closest(rtx, s, t, m, q)
    missed = int((wq["kind"] == 0).sum())
    assert len(q) // 4 < missed < 3 * len(q) // 4, missed
    cc.assert_same_records(rtx, tr.closest_points(q), wq, what + ", R = the median distance")


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, p, want = cases(name)
    assert (want["dst"][:-3] >= 0).all() and (name == "spheres" or (want["dst"] == 0).sum() >= 1)       # zero distances are in
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_batch(rtx, tr, s, t, m, p, want, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")
        if name == "plane":
            assert tr.stats()["numBvhNodes"] > 5                # (several levels)


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("plane", "Knight"):
        s, t, m, p, want = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            cc.assert_same_records(rtx, tr.closest_points(p), want, f"{name} max_leaf {max_leaf}")


@pytest.mark.parametrize("name", ["two", "mixed", "Knight"])
def test_scene_and_points_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): distances stay small while coordinates are large"""
    s, t, m, p, _ = cases(name)
    off = np.array([1e4, -1e4, 1e4], np.float32)
    s2, t2, m2, p2 = s.copy(), t.copy(), m.copy(), p.copy()
    s2["position"] += off
    for k in ("posA", "posB", "posC"):
        t2[k] += off
    m2["boundsMin"] += off
    m2["boundsMax"] += off
    p2["origin"] += off
    want = cc.oracle_closest(rtx, s2, t2, m2, p2)
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            check_batch(rtx, tr, s2, t2, m2, p2, want, f"{name} translated, compact_nodes {compact_nodes}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, p, want = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        cc.assert_same_records(rtx, tr.closest_points(p), want, f"lds_stack 3, compact_nodes {compact_nodes}")
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        p = batch_of(rtx, s, world, infos, seed=5)
        got = tr.closest_points(p)
        cc.assert_same_records(rtx, got, cc.oracle_closest(rtx, s, world, infos, p, chunk_mesh), f"local meshes, device_bvh {device_bvh}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_slices_split_calls_and_counting_are_invisible(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        tr.set_option("closest_slice", 100)
        cc.assert_same_records(rtx, tr.closest_points(p), want, "closest_slice 100")
        tr.set_option("closest_slice", 1 << 22)
        for cut in (1, 333):
            cc.assert_same_records(rtx, np.concatenate([tr.closest_points(p[:cut]), tr.closest_points(p[cut:])]), want, f"cut at {cut}")
        assert tr.closest_info()["lastPrimTests"] == 0 and tr.closest_info()["lastNodeSteps"] == 0
        tr.set_option("closest_count", 1)
        cc.assert_same_records(rtx, tr.closest_points(p), want, "the counting kernel")
        info = tr.closest_info()
        searched = int((p["tMax"] > 0).sum())
        assert info["lastPrimTests"] >= searched * len(s) and info["lastNodeSteps"] >= searched, info
        assert info["calls"] == 6 and info["lastKernelMs"] > 0 and info["totalKernelMs"] > info["lastKernelMs"], info
        lib = rtx.load_library()
        assert lib.rt_set_option(tr._ctx, b"closest_slice", 0) == -2 and lib.rt_set_option(tr._ctx, b"closest_count", 2) == -2


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        cc.assert_same_records(rtx, mt.closest_points(p), want, "two contexts")
        cc.assert_same_records(rtx, mt.closest_points(p[:1]), want[:1], "fewer points than contexts")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/closest_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "closest_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "closest device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals(rtx, cases):
    """(label, call, code, a word of the message); the misaligned device pointer is in the torch worker, which has device memory"""
    s, t, m, p, _ = cases("mixed")
    lib = rtx.load_library()
    r = np.ascontiguousarray(p[:8])
    out = np.zeros(8, rtx.CLOSEST)
    out["dst"] = 7.0
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert lib.rt_closest_points(None, vp(r), 8, vp(out)) == -1 and lib.rt_closest_points_device(None, vp(r), 8, vp(out)) == -1
    assert lib.rt_multi_closest_points(None, vp(r), 8, vp(out)) == -1 and lib.rt_get_closest_info(None, None) == -1
    with tracer_of(rtx, s, t, m) as tr, rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        c, h = tr._ctx, mt._m
        stats = tr.stats()
        table = [
            ("host, n < 0", lambda: lib.rt_closest_points(c, vp(r), -1, vp(out)), -2, b"bad arguments"),
            ("host, null points", lambda: lib.rt_closest_points(c, None, 8, vp(out)), -2, b"points"),
            ("host, null out", lambda: lib.rt_closest_points(c, vp(r), 8, None), -2, b"out"),
            ("host, n == 0", lambda: lib.rt_closest_points(c, vp(r), 0, None), 0, b""),
            ("host, n == 0 and nothing", lambda: lib.rt_closest_points(c, None, 0, None), 0, b""),
            ("device, n < 0", lambda: lib.rt_closest_points_device(c, vp(r), -1, vp(out)), -2, b"bad arguments"),
            ("device, null points", lambda: lib.rt_closest_points_device(c, None, 8, vp(out)), -2, b"points"),
            ("device, null out", lambda: lib.rt_closest_points_device(c, vp(r), 8, None), -2, b"out"),
            ("device, n == 0", lambda: lib.rt_closest_points_device(c, None, 0, None), 0, b""),
            ("device, host memory", lambda: lib.rt_closest_points_device(c, vp(r), 8, vp(out)), -2, b"device"),
            ("info, null out", lambda: lib.rt_get_closest_info(c, None), -1, b""),
            ("multi, n < 0", lambda: lib.rt_multi_closest_points(h, vp(r), -1, vp(out)), -2, b"bad arguments"),
            ("multi, null points", lambda: lib.rt_multi_closest_points(h, None, 8, vp(out)), -2, b"points"),
            ("multi, null out", lambda: lib.rt_multi_closest_points(h, vp(r), 8, None), -2, b"out"),
            ("multi, n == 0", lambda: lib.rt_multi_closest_points(h, vp(r), 0, None), 0, b""),
        ]
        for label, call, code, word in table:
            assert call() == code, label
            if code == -2:
                msg = lib.rt_multi_last_error(h) if label.startswith("multi") else lib.rt_last_error(c)
                assert word in msg and b"rt_" in msg, (label, msg)
        assert (out["dst"] == 7.0).all()
        info = tr.closest_info()
        assert info["calls"] == 0 and info["lastKernelMs"] == 0 and info["totalKernelMs"] == 0, info
        assert all(np.array_equal(v, tr.stats()[k]) for k, v in stats.items())


STATS_MAY_MOVE = ("bvhBuilds", "bvhRebuilds", "bvhRepads")


def test_a_call_moves_no_other_state(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    params, s, t, m = mgr.build_buffers()
    _, _, _, p, want = cases("mixed")
    K = 2
    with rtx.Tracer(0) as ta:
        ta.set_params(params)
        ta.upload(spheres=s, triangles=t, meshinfo=m)
        ta.render(0, 2 * K)
        image = ta.read_accum()
    with rtx.Tracer(0) as tb:
        tb.set_params(params)
        tb.upload(spheres=s, triangles=t, meshinfo=m)
        tb.render(0, K)
        tb.render_aov(0, 2)
        tb.denoise(iterations=2)
        tb.temporal()
        tb.visibility(p[:64], 4)

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "gather_info": tb.gather_info(), "visibility_info": tb.visibility_info(),
                    "stats": tb.stats()}
        before = state()
        assert tb.closest_info()["calls"] == 0
        cc.assert_same_records(rtx, tb.closest_points(p), want, "beside an image")       # (the far points widen the padding)
        assert tb.closest_info()["calls"] == 1
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info", "visibility_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            tb.closest_points(p[:100])
        assert tb.read_accum().tobytes() == image.tobytes()


def test_manager_method(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    _, _, _, p, want = cases("mixed")
    with rtx.Tracer(0) as tr:
        mgr.backend = tr
        cc.assert_same_records(rtx, mgr.ClosestPoints(p), want, "RayTracingManager.ClosestPoints")


def test_the_traversal_prunes(rtx):
    """8192 triangles, 4096 points one cell above them: brute force is 8192 tests a point; a traversal needs a small fraction.  The bound
    (one sixteenth) separates a traversal from a scan; it is not a speed target."""
    s, t, m = plane(rtx, 64, 64)
    cell = 8.0 / 64
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.uniform(0, 8, (4096, 2)), np.full((4096, 1), cell)], 1)
    p = cc.points_of(rtx, xyz)
    want, brute = cc.oracle_closest(rtx, s, t, m, p, count=True)
    assert brute == 4096 * 8192
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, closest_count=1) as tr:
            cc.assert_same_records(rtx, tr.closest_points(p), want, "plane of 8192")
            info = tr.closest_info()
            print(f"compact_nodes {compact_nodes}: prim tests / point {info['lastPrimTests'] / 4096:.2f}, node steps / point {info['lastNodeSteps'] / 4096:.2f}")
            assert 0 < info["lastPrimTests"] / 4096 < 512, info
