"""K-nearest point queries on the GPU (rt_closest_points and its device and rt_multi forms with the options "closest_k" and
"closest_all"): every word of every record bit for bit against the brute-force checker (tests/nearest_oracle.c, pinned by
tests/test_nearest_cpu.py), over test_gpu_closest's scenes and batches extended by points above shared vertices (whose K-th and
(K+1)-th keys tie), in the forms (K, all) = (2, 0), (8, 0), (3, 1), (1, 1): both node forms, both builders, every leaf size, scenes far
from the origin, a traversal stack that spills, a refitted local-mesh scene, invisible slicing, rt_multi, the device entry; refusals;
the defaults; the state a call leaves alone; that the K-th key prunes; the host methods."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
import nearest_check as nc
from listed_gpu import ask, check_a_call_moves_no_other_state, check_forms, check_split_calls_and_counting, make_cases
from ray_query_helpers import scene_of
from test_gpu_closest import NAMES, batch_of, buffers_of, plane, tracer_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, points, {(K, all): the checker's answer}), each computed once"""
    return make_cases(rtx, "nearest", buffers_of)


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, p, want = cases(name)
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_forms(rtx, tr, "nearest", p, want, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")
        if name == "plane":
            assert tr.stats()["numBvhNodes"] > 5                # (several levels)


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("plane", "Knight"):
        s, t, m, p, want = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            check_forms(rtx, tr, "nearest", p, want, f"{name} max_leaf {max_leaf}", [(8, 0)])


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
    want = {f: nc.oracle_nearest(rtx, s2, t2, m2, p2, *f) for f in ((8, 0), (3, 1))}
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            check_forms(rtx, tr, "nearest", p2, want, f"{name} translated, compact_nodes {compact_nodes}", list(want))


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, p, want = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        check_forms(rtx, tr, "nearest", p, want, f"lds_stack 3, compact_nodes {compact_nodes}", [(8, 0), (3, 1)])
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        p = nc.batch_of(rtx, s, world, infos, batch_of(rtx, s, world, infos, seed=5))
        for f in ((8, 0), (3, 1)):
            got = ask(tr, "nearest", p, *f)
            nc.assert_same_records(rtx, got, nc.oracle_nearest(rtx, s, world, infos, p, *f, chunk_mesh=chunk_mesh), f"local meshes, device_bvh {device_bvh}, {f}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_slices_split_calls_and_counting_are_invisible(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        tr.set_option("closest_slice", 100)
        check_forms(rtx, tr, "nearest", p, want, "closest_slice 100")
        tr.set_option("closest_slice", 333)
        check_forms(rtx, tr, "nearest", p, want, "closest_slice 333", [(8, 0)])
        searched = int((p["tMax"] > 0).sum())
        check_split_calls_and_counting(rtx, "nearest", tr, p, want,
                                       lambda info: info["lastPrimTests"] >= searched * len(s) and info["lastNodeSteps"] >= searched)


def test_a_batch_longer_than_the_effective_slice_at_k_8(rtx):
    """524288 + 3 points at K = 8: more than min(closest_slice, 4194304 / K) = 524288, so the call takes two launches and two staging
    slices, and the records on either side of the cut are the bits of a call on those points alone.  (This shows the cut is invisible;
    it would pass with an unreduced slice as well — that the slice IS reduced is closest_call's one line, not something a result shows.)"""
    s, t, m = plane(rtx, 2, 2)
    n = (1 << 22) // 8 + 3
    rng = np.random.default_rng(8)
    p = cc.points_of(rtx, rng.uniform(-1, 9, (n, 3)).astype(np.float32), 3.0)
    with tracer_of(rtx, s, t, m) as tr:
        got = ask(tr, "nearest", p, 8, 0)
        assert got.shape == (n, 8)
        edge = np.r_[0:64, n - 67:n]
        nc.assert_same_records(rtx, got[edge], nc.oracle_nearest(rtx, s, t, m, p[edge], 8, 0), "around the cut at 524288")
        nc.assert_same_records(rtx, got[edge], ask(tr, "nearest", p[edge], 8, 0), "the same points alone")


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with rtx.MultiTracer([0] * 3) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        check_forms(rtx, mt, "nearest", p, want, "three contexts")
        nc.assert_same_records(rtx, ask(mt, "nearest", p[:1], 8, 0), want[8, 0][:1], "fewer points than contexts")
        cc.assert_same_records(rtx, mt.closest_points(p), cc.oracle_closest(rtx, s, t, m, p), "three contexts, the defaults")


def test_device_entry_on_tensors_matches_the_checker():
    """(in a fresh process that imports torch first: tests/listed_torch_worker.py nearest)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "listed_torch_worker.py"), "nearest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nearest device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals_leave_the_options_and_every_state_alone(rtx, cases):
    s, t, m, p, want = cases("mixed")
    lib = rtx.load_library()
    with tracer_of(rtx, s, t, m) as tr, rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        tr.set_option("closest_k", 3)
        tr.set_option("closest_all", 1)
        mt.set_option("closest_k", 3)
        mt.set_option("closest_all", 1)
        stats, info = tr.stats(), tr.closest_info()
        for name, value, word in ((b"closest_k", 0, b"closest_k"), (b"closest_k", 9, b"closest_k"), (b"closest_k", -1, b"closest_k"),
                                  (b"closest_all", 2, b"closest_all"), (b"closest_all", -1, b"closest_all")):
            assert lib.rt_set_option(tr._ctx, name, value) == -2 and word in lib.rt_last_error(tr._ctx), (name, value)
            assert lib.rt_multi_set_option(mt._m, name, value) == -2 and word in lib.rt_multi_last_error(mt._m), (name, value)
        assert all(np.array_equal(v, tr.stats()[k]) for k, v in stats.items()) and tr.closest_info() == info
        # the options kept their values: the next call is still (3, 1)
        nc.assert_same_records(rtx, tr.closest_points(p).reshape(len(p), 3), want[3, 1], "after the refusals")
        nc.assert_same_records(rtx, mt.closest_points(p).reshape(len(p), 3), want[3, 1], "rt_multi after the refusals")


def test_the_defaults_are_todays_bytes(rtx, cases):
    s, t, m, p, want = cases("mixed")
    default = cc.oracle_closest(rtx, s, t, m, p)
    with tracer_of(rtx, s, t, m) as tr:
        got = tr.closest_points(p)
        assert got.shape == (len(p),) and (got["_reserved"] == 0).all()
        cc.assert_same_records(rtx, got, default, "before any option")
        check_forms(rtx, tr, "nearest", p, want, "in between")
        tr.set_option("closest_k", 1)
        tr.set_option("closest_all", 0)
        again = tr.closest_points(p)
        assert again.shape == (len(p),) and again.tobytes() == got.tobytes()
        for f in nc.FORMS:
            nc.assert_first_is_the_default(rtx, ask(tr, "nearest", p, *f), got, f"{f}")


def test_a_call_moves_no_other_state(rtx, cases):
    _, _, _, p, want = cases("mixed")

    def every_other_call_ignores_the_options(tb):               # the same hits, rays and frame with them set
        hits, rays = tb.trace_hits(p[:64], 4), tb.trace_rays(p[:64])
        tb.set_option("closest_k", 8)
        tb.set_option("closest_all", 1)
        assert tb.trace_hits(p[:64], 4).tobytes() == hits.tobytes() and tb.trace_rays(p[:64]).tobytes() == rays.tobytes()
    check_a_call_moves_no_other_state(rtx, "nearest", p, want, every_other_call_ignores_the_options)   # (the far points widen the padding)


def test_the_kth_key_prunes_and_the_radius_alone_does_not(rtx):
    """8192 triangles, 1024 points one cell above them, R unbounded.  all = 1: nothing can be culled, so every point tests every triangle
    of the tree, exactly.  K = 8, all = 0: the 8th key bounds the walk, and the count is strictly smaller."""
    s, t, m = plane(rtx, 64, 64)
    rng = np.random.default_rng(3)
    n = 1024
    p = cc.points_of(rtx, np.concatenate([rng.uniform(0, 8, (n, 2)), np.full((n, 1), 8.0 / 64)], 1))
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, closest_count=1) as tr:
            nc.assert_same_records(rtx, ask(tr, "nearest", p, 1, 1), nc.oracle_nearest(rtx, s, t, m, p, 1, 1), "plane of 8192, (1, 1)")
            everything = tr.closest_info()
            assert everything["lastPrimTests"] == n * (len(s) + len(t)), everything
            nc.assert_same_records(rtx, ask(tr, "nearest", p, 8, 0), nc.oracle_nearest(rtx, s, t, m, p, 8, 0), "plane of 8192, (8, 0)")
            pruned = tr.closest_info()
            print(f"compact_nodes {compact_nodes}: prim tests / point {pruned['lastPrimTests'] / n:.2f} at (8, 0) against {everything['lastPrimTests'] / n:.0f} at (1, 1); "
                  f"node steps / point {pruned['lastNodeSteps'] / n:.2f} against {everything['lastNodeSteps'] / n:.2f}")
            assert 0 < pruned["lastPrimTests"] < everything["lastPrimTests"] and pruned["lastNodeSteps"] < everything["lastNodeSteps"]


def test_host_methods(rtx, cases):
    s, t, m, p, want = cases("mixed")
    mgr = scene_of(rtx, "mesh_test_scene")
    with rtx.Tracer(0) as tr:
        mgr.backend = tr
        nc.assert_same_records(rtx, mgr.OverlapSphere(p, maxResults=3), want[3, 1], "RayTracingManager.OverlapSphere")
        nc.assert_same_records(rtx, mgr.OverlapSphere(p, maxResults=8, countAll=False), want[8, 0], "RayTracingManager.OverlapSphere, countAll False")
        for k, count_all in nc.FORMS:
            got = rtx.nearest.nearest_k(tr, p, k, count_all=bool(count_all))
            assert got.shape == (len(p), k)
            nc.assert_same_records(rtx, got, want[k, count_all], f"nearest_k {k} {count_all}")
        R = np.float32(1.5)
        q = p.copy()
        q["tMax"] = R
        counts = rtx.nearest.overlap_count(tr, p, R)
        assert counts.dtype == np.int32 and counts.shape == (len(p),)
        assert np.array_equal(counts, nc.oracle_nearest(rtx, s, t, m, q, 1, 1)["_reserved"][:, 0, 0]) and counts.max() > 8
        assert (p["tMax"] != R).any()                               # (the caller's points are left alone)
        cc.assert_same_records(rtx, tr.closest_points(p), cc.oracle_closest(rtx, s, t, m, p), "the defaults are back")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        nc.assert_same_records(rtx, rtx.nearest.nearest_k(mt, p, 8), want[8, 0], "nearest_k on a MultiTracer")


def test_the_compiled_host_overlap_sphere(rtx, tmp_path):
    """RayTracingManager::OverlapSphere of the compiled host through its C entry rth_overlap_sphere (no CppScene method reaches it: the
    Python window's surface is a recorded one), on a fresh rt_ctx and on an rt_multi of three: the non-empty records and the total
    against the checker at (K, all) = (max_results, 1), a point with nothing in range, and the host's next ClosestPoints the default
    call again."""
    from rtx_amd import unity_scene
    from rtx_amd.host_cpp_binding import CppScene
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    path = str(tmp_path / "scene.unity")
    unity_scene.save_unity_scene(mgr, path)
    cpp = CppScene(path, 64, 48)
    try:
        _, s, t, m = cpp.build_buffers()
        L = cpp._L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.rth_overlap_sphere.argtypes = [vp, ctypes.POINTER(ci), ci, vp, ctypes.c_float, ci, vp, ctypes.POINTER(ci)]
        L.rth_overlap_sphere.restype = ci
        lo, hi = t["posA"].min(0), t["posA"].max(0)
        rng = np.random.default_rng(21)
        centres = np.concatenate([t["posA"][rng.integers(0, len(t), 6)], (lo + rng.random((6, 3)) * (hi - lo)).astype(np.float32),
                                  s["position"][:2] + np.float32([0, 0.25, 0])]).astype(np.float32)
        R = np.float32(np.linalg.norm(hi - lo) / 6)
        cases = [(c, R, k) for c, k in zip(centres, (8, 3, 1, 5, 8, 2, 8, 4, 1, 8, 6, 8, 8, 3))]
        cases.append((np.float32(hi + (hi - lo) * 100), R, 4))             # nothing within reach
        cases.append((centres[0], np.float32(np.inf), 8))                    # everything within reach: total = every primitive
        seen_none = seen_more = 0
        for devices in ((), (0, 0, 0)):
            devs = (ci * max(len(devices), 1))(*(devices or (0,)))
            for centre, radius, k in cases:
                out = np.zeros(8, rtx.CLOSEST)
                out["dst"] = 7.0
                total = ci(-5)
                c = np.ascontiguousarray(centre, np.float32)
                n = L.rth_overlap_sphere(cpp._h, devs, len(devices), c.ctypes.data_as(vp), float(radius), k, out.ctypes.data_as(vp), ctypes.byref(total))
                assert n >= 0, L.rth_last_error()
                want = nc.oracle_nearest(rtx, s, t, m, cc.points_of(rtx, [centre], radius), k, 1)[0]
                found = int((want["kind"] != 0).sum())
                what = f"devices {devices}, centre {centre}, R {radius}, max_results {k}"
                assert n == found and total.value == int(want["_reserved"][0, 0]), (what, n, found, total.value)
                nc.assert_same_records(rtx, out[:n], want[:n], what)
                assert (out["dst"][n:] == 7.0).all(), what                   # (only the non-empty records are written)
                seen_none += n == 0
                seen_more += total.value > k
            p = cc.points_of(rtx, centres, R)
            cc.assert_same_records(rtx, cpp.closest_points(p, devices=devices), cc.oracle_closest(rtx, s, t, m, p), f"ClosestPoints afterwards, devices {devices}")
        assert seen_none >= 2 and seen_more >= 4 and total.value > 8      # (the last case: R = +inf, everything counted)
        assert L.rth_overlap_sphere(cpp._h, None, 0, centres.ctypes.data_as(vp), 1.0, 9, out.ctypes.data_as(vp), None) == -1
    finally:
        cpp.close()
