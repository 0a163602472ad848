"""Sphere-cast-all on the GPU (option "hits_sweep" = 1 on rt_trace_hits, its device and rt_multi forms; sweep.sphere_cast_all): every word
of every record against the brute-force checker (tests/sweep_all_oracle.c, pinned by tests/test_sweep_all_cpu.py), on
test_gpu_closest.py's scenes with sweep_check.batch_of's 710 rays.  Both node forms, both builders, every leaf size, K in {1, 2, 3, 8}
with and without countAll, coordinates far from the origin, a traversal stack that spills, a refitted local-mesh scene, tMax in the
middle of the lists, batches cut into two calls, launches cut by "hits_slice", rt_multi, the device entry; cross-checks against the
sphere casts on the device alone; the option's refusal; what the option leaves alone at 0 and at 1; the state a call leaves alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
import sweep_all_check as sac
import sweep_check as sc
from ray_query_helpers import scene_of
from test_gpu_closest import STATS_MAY_MOVE, buffers_of, tracer_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("one", "two", "plane", "spheres", "mixed", "Knight")
FORMS = [(K, ca) for K in sac.KS for ca in (False, True)]


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, rays, want): want(K, count_all) is the checker's list, each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            rays, _ = sc.batch_of(rtx, s, t, m)
            rays.setflags(write=False)
            lists = {}

            def want(K, count_all, lists=lists, scene=(s, t, m), rays=rays):
                if (K, count_all) not in lists:
                    lists[K, count_all] = sac.oracle_cast_all(rtx, *scene, rays, K, count_all)
                    lists[K, count_all].setflags(write=False)
                return lists[K, count_all]
            cache[name] = (s, t, m, rays, want)
        return cache[name]
    return get


def cast_all(rtx, tr, rays, K=4, count_all=False):
    return rtx.sweep.sphere_cast_all(tr, rays, sc.radii_of(rays), K, count_all)


def check_forms(rtx, tr, rays, want, forms, what):
    for K, ca in forms:
        got = cast_all(rtx, tr, rays, K, ca)
        assert got.shape == (len(rays), K)
        sac.assert_same_records(rtx, got, want(K, ca), f"{what}, K {K}, countAll {ca}")
        assert (got["kind"][-sc.N_UNTRACED:] == 0).all() and (got["hitCount"][-sc.N_UNTRACED:] == 0).all()


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, rays, want = cases(name)
    forms = FORMS if name in ("mixed", "Knight") else [(8, True), (2, False)]
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_forms(rtx, tr, rays, want, forms, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("plane", "Knight"):
        s, t, m, rays, want = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            check_forms(rtx, tr, rays, want, [(8, False), (3, True)], f"{name} max_leaf {max_leaf}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, rays, want = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        check_forms(rtx, tr, rays, want, [(8, True), (2, False)], f"lds_stack 3, compact_nodes {compact_nodes}")
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("name", ["two", "mixed", "Knight"])
def test_scene_and_rays_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): the balls stay small while coordinates are large"""
    s, t, m, rays, _ = cases(name)
    off = np.array([1e4, -1e4, 1e4], np.float32)
    s2, t2, m2, r2 = s.copy(), t.copy(), m.copy(), rays.copy()
    s2["position"] += off
    for k in ("posA", "posB", "posC"):
        t2[k] += off
    m2["boundsMin"] += off
    m2["boundsMax"] += off
    r2["origin"] += off
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            for K, ca in ((8, False), (3, True)):
                sac.assert_same_records(rtx, cast_all(rtx, tr, r2, K, ca), sac.oracle_cast_all(rtx, s2, t2, m2, r2, K, ca),
                                        f"{name} translated, compact_nodes {compact_nodes}, K {K}")


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        rays, _ = sc.batch_of(rtx, s, world, infos, seed=5)
        for K, ca in ((8, True), (2, False)):
            got = cast_all(rtx, tr, rays, K, ca)
            sac.assert_same_records(rtx, got, sac.oracle_cast_all(rtx, s, world, infos, rays, K, ca, chunk_mesh), f"local meshes, device_bvh {device_bvh}, K {K}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_tmax_at_the_median_dst(rtx, cases):
    """the contacts beyond it leave the lists and the counts, the others keep their bits"""
    s, t, m, rays, want = cases("mixed")
    full = want(8, True)
    q = rays.copy()
    q["tMax"][:-sc.N_UNTRACED] = np.median(full["dst"][np.isfinite(full["dst"])])
    with tracer_of(rtx, s, t, m) as tr:
        for K, ca in ((8, True), (2, False)):
            wq = sac.oracle_cast_all(rtx, s, t, m, q, K, ca)
            assert 0 < (wq["kind"] != 0).sum() < (want(K, ca)["kind"] != 0).sum()
            sac.assert_same_records(rtx, cast_all(rtx, tr, q, K, ca), wq, f"tMax = the median dst, K {K}")


def test_cut_batches_slices_and_the_options_refusal(rtx, cases):
    s, t, m, rays, want = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        for cut in (1, 333):
            sac.assert_same_records(rtx, np.concatenate([cast_all(rtx, tr, rays[:cut], 3, True), cast_all(rtx, tr, rays[cut:], 3, True)]), want(3, True), f"cut at {cut}")
        lib = rtx.load_library()
        plain = tr.trace_hits(rays, 4)
        assert lib.rt_set_option(tr._ctx, b"hits_sweep", 2) == -2 and b"hits_sweep" in lib.rt_last_error(tr._ctx)
        assert lib.rt_set_option(tr._ctx, b"hits_sweep", -1) == -2
        # the option kept its value, 0: the same rays are plain rays, and the next cast is the checker's
        assert tr.trace_hits(rays, 4).tobytes() == plain.tobytes()
        sac.assert_same_records(rtx, cast_all(rtx, tr, rays, 8, False), want(8, False), "after the refusals")
        assert tr.trace_hits(rays, 4).tobytes() == plain.tobytes()
        # ... and at 1 a refusal leaves it at 1
        tr.set_option("hits_sweep", 1)
        assert lib.rt_set_option(tr._ctx, b"hits_sweep", 2) == -2
        sac.assert_same_records(rtx, tr.trace_hits(rays, 2), want(2, False), "set by hand, after a refusal")
        # "sweep" is independent of it: either may be 0 or 1
        tr.set_option("sweep", 1)
        sac.assert_same_records(rtx, tr.trace_hits(rays, 2), want(2, False), "both options at 1")
        tr.set_option("hits_sweep", 0)
        assert tr.trace_hits(rays, 4).tobytes() == plain.tobytes()
        tr.set_option("sweep", 0)
        # the library's slices are invisible: a launch per 100 rays, the last one of 10
        tr.set_option("hits_slice", 100)
        sac.assert_same_records(rtx, cast_all(rtx, tr, rays, 8, True), want(8, True), "hits_slice 100")
        info = tr.hits_info()
        assert (info["lastMaxHits"], info["lastMode"], info["lastCountAll"]) == (8, rtx.HITS_FRONT, 1)
    with tracer_of(rtx, s, t, m) as tr:
        sac.assert_same_records(rtx, cast_all(rtx, tr, rays[:100], 8, False), want(8, False)[:100], "100 rays")
        # the params' mode is validated as ever and then not read
        tr.set_option("hits_sweep", 1)
        sac.assert_same_records(rtx, tr.trace_hits(rays, 3, both_sides=True), want(3, False), "RT_HITS_BOTH")
        assert tr.hits_info()["lastMode"] == rtx.HITS_BOTH
        p = np.zeros((), rtx.HITS_PARAMS)
        p["maxHits"], p["mode"] = 3, 2
        out = np.zeros((len(rays), 3), rtx.MULTIHIT)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
        assert lib.rt_trace_hits(tr._ctx, vp(rays), len(rays), vp(p), vp(out)) == -2
        p["mode"], p["_reserved"] = 0, 1
        assert lib.rt_trace_hits(tr._ctx, vp(rays), len(rays), vp(p), vp(out)) == -2      # (a reserved word: refused unless 0)
        p["_reserved"] = 0
        assert lib.rt_trace_hits(tr._ctx, vp(rays), len(rays), vp(p), vp(out)) == 0
        sac.assert_same_records(rtx, out, want(3, False), "through the C entry")


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, rays, want = cases("mixed")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        sac.assert_same_records(rtx, cast_all(rtx, mt, rays, 8, True), want(8, True), "two contexts")
        sac.assert_same_records(rtx, cast_all(rtx, mt, rays, 2, False), want(2, False), "two contexts")
    with rtx.MultiTracer([0] * 3) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        sac.assert_same_records(rtx, cast_all(rtx, mt, rays[:2], 8, True), want(8, True)[:2], "more contexts than rays")
        sac.assert_same_records(rtx, cast_all(rtx, mt, rays, 3, True), want(3, True), "three contexts")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/sweep_torch_worker.py cast_all)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "sweep_torch_worker.py"), "cast_all"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep-all device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", ["mixed", "Knight", "spheres"])
def test_record_0_is_the_sphere_cast_and_the_count_is_the_sphere_check(rtx, cases, name):
    """on the device alone, no checker: words 0..12 and the feature code of record 0, and hitCount > 0 exactly where sphere_check says 1"""
    s, t, m, rays, _ = cases(name)
    r = sc.radii_of(rays)
    with tracer_of(rtx, s, t, m) as tr:
        first, occ = rtx.sweep.sphere_cast(tr, rays, r), rtx.sweep.sphere_check(tr, rays, r)
        wf = first.view(np.uint32).reshape(-1, 16)
        for K, ca in ((1, False), (4, False), (8, True)):
            got = cast_all(rtx, tr, rays, K, ca)
            w = sac.words(got[:, 0])
            assert np.array_equal(w[:, :13], wf[:, :13]) and np.array_equal(w[:, 15], wf[:, 13]), (name, K, ca)
            assert np.array_equal(got[:, 0]["hitCount"] > 0, occ == 1) and (got["hitCount"] == got[:, :1]["hitCount"]).all()
        # a call at K holds the first K records of a call at a larger K
        a, b = sac.words(cast_all(rtx, tr, rays, 3, True)).copy(), sac.words(cast_all(rtx, tr, rays, 8, True)[:, :3]).copy()
        assert np.array_equal(a, b)


def test_with_the_option_at_0_rt_trace_hits_keeps_its_bits(rtx, cases):
    """before and after a sphere-cast-all, on rays whose reserved word holds radii, and garbage"""
    s, t, m, rays, want = cases("mixed")
    junk = rays.copy()
    junk["_reserved"][::2] = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31 - 1, len(junk[::2]))
    clean = rays.copy()
    clean["_reserved"] = 0

    def plain(tr, r):
        return (tr.trace_hits(r, 4, both_sides=True), tr.trace_hits(r, 8, count_all=True), tr.trace_hits(r, 1))
    with tracer_of(rtx, s, t, m) as tr:
        before = plain(tr, clean)
        sac.assert_same_records(rtx, cast_all(rtx, tr, rays, 8, True), want(8, True), "the cast in between")
        for r in (clean, rays, junk):
            for a, b in zip(before, plain(tr, r)):
                assert a.tobytes() == b.tobytes()
        assert (before[0]["_reserved"] == 0).all() and (before[0]["kind"] != 0).any()


def test_the_option_at_1_leaves_the_other_calls_alone(rtx, cases):
    s, t, m, rays, _ = cases("mixed")
    p = cc.points_of(rtx, rays["origin"][:64], 1.0)
    pts = rays[:64].copy()
    pts["tMax"] = 2.0
    def others(tr):
        return (tr.trace_rays(rays), tr.occluded(rays), tr.closest_points(p), tr.visibility(pts, 4), rtx.sweep.sphere_cast(tr, rays, sc.radii_of(rays)))
    with tracer_of(rtx, s, t, m) as tr:
        at0 = others(tr)
        tr.set_option("hits_sweep", 1)
        at1 = others(tr)
        tr.set_option("hits_sweep", 0)
        for a, b in zip(at0, at1):
            assert a.tobytes() == b.tobytes()
        assert (at0[0]["kind"] != 0).any() and at0[1].any() and (at0[4]["kind"] != 0).any()


def test_a_call_moves_no_other_state(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    params, s, t, m = mgr.build_buffers()
    _, _, _, rays, want = cases("mixed")
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
        tb.closest_points(cc.points_of(rtx, rays["origin"][:64]))

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "gather_info": tb.gather_info(), "visibility_info": tb.visibility_info(),
                    "closest_info": tb.closest_info(), "hits_info": tb.hits_info(), "stats": tb.stats()}
        before = state()
        sac.assert_same_records(rtx, cast_all(rtx, tb, rays, 8, True), want(8, True), "beside an image")     # (the far rays widen the padding)
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info", "visibility_info", "closest_info"):
            assert before[k] == after[k], k
        assert after["hits_info"]["calls"] == before["hits_info"]["calls"] + 1 and after["hits_info"]["lastMaxHits"] == 8
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            cast_all(rtx, tb, rays[:100], 4)
        assert tb.read_accum().tobytes() == image.tobytes()
