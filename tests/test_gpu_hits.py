"""Multi-hit ray queries on the GPU (rt_trace_hits and its device and rt_multi forms): every field of every record bit for bit against
the brute-force checker (tests/hits_oracle.c, pinned by tests/test_hits_cpu.py), over the smallest scenes that can still go wrong — the
closest-point tests' seven, twelve stacked planes whose rays cross more than eight surfaces (evictions) and concentric shells (entry /
exit pairs) — with K in {1, 2, 3, 8}, both modes, both countAll values and both intersect modes, both node forms, both builders, every
leaf size, a traversal stack that spills, scenes 1e4 from the origin, a refitted local-mesh scene, invisible slicing and rt_multi, the
device entry; ray by ray against rt_trace_rays and rt_occluded; refusals; the state a call leaves alone; the manager's RaycastAll.

Every scene's batch is hits_check.batch_of's (about 2900 rays: random rays of any length, rays aimed at shared edges and vertices,
origins on surfaces, tMax of 0, -1, NaN, 1e-6, exactly a hit's dst and the float after it, NaN / inf components, zero directions)."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import hits_check as hc
from ray_query_helpers import scene_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 3, 8)
FORMS = list(itertools.product(KS, (hc.FRONT, hc.BOTH), (False, True)))       # (K, mode, countAll)


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, rays), and (name, K, mode, countAll, intersect) -> the checker's answer, each computed once"""
    scenes, answers = {}, {}

    def scene(name):
        if name not in scenes:
            s, t, m = hc.buffers_of(rtx, name)
            rays = hc.batch_of(rtx, s, t, m)
            rays.setflags(write=False)
            scenes[name] = (s, t, m, rays)
        return scenes[name]

    def want(name, K, mode, count_all, intersect=0):
        key = (name, K, mode, count_all, intersect)
        if key not in answers:
            s, t, m, rays = scene(name)
            answers[key] = hc.oracle_hits(rtx, s, t, m, rays, K, mode, count_all, intersect)
            answers[key].setflags(write=False)
        return answers[key]
    scene.want = want
    return scene


def brute_params(rtx):
    """rt_params whose only purpose is intersectMode = RT_INTERSECT_BRUTE"""
    params = scene_of(rtx, "mesh_test_scene").build_buffers()[0]
    params["intersectMode"] = rtx.RT_INTERSECT_BRUTE
    return params


def tracer_of(rtx, s, t, m, intersect=0, **options):
    tr = rtx.Tracer(0)
    for k, v in options.items():
        tr.set_option(k, v)
    if intersect:
        tr.set_params(brute_params(rtx))                        # (FLAT_CHUNKS needs no params at all)
    tr.upload(spheres=s, triangles=t, meshinfo=m)
    return tr


def check_forms(rtx, tr, cases, name, intersect, what, forms=FORMS):
    rays = cases(name)[3]
    for K, mode, count_all in forms:
        got = tr.trace_hits(rays, K, mode == hc.BOTH, count_all)
        assert got.shape == (len(rays), K)
        hc.assert_same_records(rtx, got, cases.want(name, K, mode, count_all, intersect), f"{what}, K {K} mode {mode} countAll {count_all}")


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("name", hc.SCENES)
def test_scenes_all_forms_and_intersect_modes(rtx, cases, name, intersect):
    s, t, m, rays = cases(name)
    with tracer_of(rtx, s, t, m, intersect) as tr:
        check_forms(rtx, tr, cases, name, intersect, f"{name} intersect {intersect}")
        info = tr.hits_info()
        assert info["calls"] == len(FORMS) and (info["lastMaxHits"], info["lastMode"], info["lastCountAll"]) == (8, 1, 1), info
        assert info["lastKernelMs"] > 0 and info["totalKernelMs"] > info["lastKernelMs"], info
    deep = cases.want(name, 8, hc.BOTH, True, intersect)
    if name in ("layers", "shells"):
        assert (deep[:, 0]["hitCount"] > 8).sum() > 100             # the list overflows: evictions happen
    assert (deep["kind"][-8:] == 0).all()                           # zero directions hit nothing


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", ["plane", "mixed", "Knight", "layers", "shells"])
def test_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, rays = cases(name)
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name in ("plane", "layers") else 2) as tr:
        check_forms(rtx, tr, cases, name, 0, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}",
                    [(1, hc.FRONT, False), (3, hc.BOTH, False), (8, hc.BOTH, True), (2, hc.FRONT, True)])


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("layers", "Knight"):
        s, t, m, rays = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            check_forms(rtx, tr, cases, name, 0, f"{name} max_leaf {max_leaf}", [(2, hc.BOTH, False), (8, hc.FRONT, True), (3, hc.BOTH, True)])


@pytest.mark.parametrize("name", ["two", "mixed", "layers"])
def test_scene_and_rays_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): distances stay small while coordinates are large"""
    s, t, m, rays = cases(name)
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
            for K, mode, count_all in ((3, hc.BOTH, False), (8, hc.BOTH, True)):
                want = hc.oracle_hits(rtx, s2, t2, m2, r2, K, mode, count_all)
                hc.assert_same_records(rtx, tr.trace_hits(r2, K, mode == hc.BOTH, count_all), want, f"{name} translated, compact_nodes {compact_nodes}, K {K}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, rays = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        check_forms(rtx, tr, cases, "Knight", 0, f"lds_stack 3, compact_nodes {compact_nodes}", [(8, hc.BOTH, True), (2, hc.FRONT, False)])
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        rays = hc.batch_of(rtx, s, world, infos, seed=5)
        for K, mode, count_all in ((1, hc.FRONT, False), (8, hc.BOTH, True)):
            got = tr.trace_hits(rays, K, mode == hc.BOTH, count_all)
            want = hc.oracle_hits(rtx, s, world, infos, rays, K, mode, count_all, int(params["intersectMode"]), chunk_mesh)
            hc.assert_same_records(rtx, got, want, f"local meshes, device_bvh {device_bvh}, K {K}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_slices_and_split_calls_are_invisible(rtx, cases):
    s, t, m, rays = cases("layers")
    want = cases.want("layers", 3, hc.BOTH, True)
    with tracer_of(rtx, s, t, m) as tr:
        tr.set_option("hits_slice", 100)
        hc.assert_same_records(rtx, tr.trace_hits(rays, 3, True, True), want, "hits_slice 100")
        tr.set_option("hits_slice", 1 << 18)
        for cut in (1, 333):
            two = np.concatenate([tr.trace_hits(rays[:cut], 3, True, True), tr.trace_hits(rays[cut:], 3, True, True)])
            hc.assert_same_records(rtx, two, want, f"cut at {cut}")
        # params == NULL: RT_HITS_DEFAULT_MAX records, front faces, hitCount capped
        lib = rtx.load_library()
        out = np.zeros((len(rays), rtx.HITS_DEFAULT_MAX), rtx.MULTIHIT)
        r = np.ascontiguousarray(rays)
        assert lib.rt_trace_hits(tr._ctx, r.ctypes.data_as(ctypes.c_void_p), len(r), None, out.ctypes.data_as(ctypes.c_void_p)) == 0
        hc.assert_same_records(rtx, out, hc.oracle_hits(rtx, s, t, m, rays, 4, hc.FRONT, False), "params == NULL")
        assert (tr.hits_info()["lastMaxHits"], tr.hits_info()["lastMode"], tr.hits_info()["lastCountAll"]) == (4, 0, 0)
        assert lib.rt_set_option(tr._ctx, b"hits_slice", 0) == -2 and lib.rt_set_option(tr._ctx, b"hits_slice", (1 << 22) + 1) == -2


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, rays = cases("shells")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        hc.assert_same_records(rtx, mt.trace_hits(rays, 8, True, True), cases.want("shells", 8, hc.BOTH, True), "two contexts")
        hc.assert_same_records(rtx, mt.trace_hits(rays[:1], 2), cases.want("shells", 2, hc.FRONT, False)[:1], "fewer rays than contexts")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/hits_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "hits_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hits device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


SHARED = ("dst", "hitPoint", "normal", "kind", "primitive", "chunk", "mesh", "u", "v")


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("name", ["plane", "mixed", "Suzanne", "layers", "shells"])
def test_record_0_is_rt_trace_rays_and_hit_count_is_rt_occluded(rtx, cases, name, intersect):
    """ray by ray on the device's own answers; the rays whose closest dst is shared by several candidates are excluded from the record
    comparison (tests/test_hits_cpu.py caps them at 2 % of the batch), never from hit / miss"""
    import query_check
    from ray_query_helpers import load_shim
    s, t, m, rays = cases(name)
    cand = query_check.oracle_candidates(rtx, load_shim(), s, t, m, intersect, rays)
    with tracer_of(rtx, s, t, m, intersect) as tr:
        first = tr.trace_hits(rays, 1)[:, 0]
        hits = tr.trace_rays(rays)
        occ = tr.occluded(rays)
        deep = tr.trace_hits(rays, 8, False, True)[:, 0]
    assert ((first["hitCount"] > 0) == (occ != 0)).all() and ((deep["hitCount"] > 0) == (occ != 0)).all()
    assert ((first["kind"] != 0) == (hits["kind"] != 0)).all()
    clear = cand <= 1
    assert (~clear).sum() <= len(rays) // 50
    for f in SHARED:
        assert first[f][clear].tobytes() == hits[f][clear].tobytes(), (name, f)
    assert (first["dst"][~clear] == hits["dst"][~clear]).all()          # a tie is a tie in dst: only the candidate kept may differ


def test_refusals(rtx, cases):
    """(label, call, code, a word of the message); the misaligned device pointer is in the torch worker, which has device memory"""
    s, t, m, rays = cases("mixed")
    lib = rtx.load_library()
    r = np.ascontiguousarray(rays[:8])
    out = np.zeros((8, 8), rtx.MULTIHIT)
    out["dst"] = 7.0
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def P(max_hits=4, mode=0, count_all=0, reserved=None):
        p = np.zeros((), rtx.HITS_PARAMS)
        p["maxHits"], p["mode"], p["countAll"] = max_hits, mode, count_all
        if reserved is not None:
            p["_reserved"][reserved] = 1
        return p
    good = P()
    assert lib.rt_trace_hits(None, vp(r), 8, vp(good), vp(out)) == -1 and lib.rt_trace_hits_device(None, vp(r), 8, vp(good), vp(out)) == -1
    assert lib.rt_multi_trace_hits(None, vp(r), 8, vp(good), vp(out)) == -1 and lib.rt_get_hits_info(None, None) == -1
    with tracer_of(rtx, s, t, m) as tr, rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        c, h = tr._ctx, mt._m
        stats = tr.stats()
        table = []
        for label, entry, handle in (("host", lib.rt_trace_hits, c), ("device", lib.rt_trace_hits_device, c), ("multi", lib.rt_multi_trace_hits, h)):
            bad = [("maxHits 0", P(0), b"maxHits"), ("maxHits 9", P(9), b"maxHits"), ("maxHits -1", P(-1), b"maxHits"), ("mode 2", P(4, 2), b"mode"),
                   ("mode -1", P(4, -1), b"mode"), ("countAll 2", P(4, 0, 2), b"countAll"), ("countAll -1", P(4, 0, -1), b"countAll"),
                   ("reserved word 0", P(reserved=0), b"reserved"), ("reserved word 4", P(reserved=4), b"reserved")]
            for what, p, word in bad:
                table.append((f"{label}, {what}", lambda entry=entry, handle=handle, p=p: entry(handle, vp(r), 8, vp(p), vp(out)), -2, word))
            table += [
                (f"{label}, n < 0", lambda entry=entry, handle=handle: entry(handle, vp(r), -1, vp(good), vp(out)), -2, b"bad arguments"),
                (f"{label}, null rays", lambda entry=entry, handle=handle: entry(handle, None, 8, vp(good), vp(out)), -2, b"rays"),
                (f"{label}, null out", lambda entry=entry, handle=handle: entry(handle, vp(r), 8, vp(good), None), -2, b"out"),
                (f"{label}, n == 0", lambda entry=entry, handle=handle: entry(handle, None, 0, None, None), 0, b""),
            ]
        table += [("device, host memory", lambda: lib.rt_trace_hits_device(c, vp(r), 8, vp(good), vp(out)), -2, b"device"),
                  ("info, null out", lambda: lib.rt_get_hits_info(c, None), -1, b"")]
        for label, call, code, word in table:
            assert call() == code, label
            if code == -2:
                msg = lib.rt_multi_last_error(h) if label.startswith("multi") else lib.rt_last_error(c)
                assert word in msg and b"rt_" in msg, (label, msg)
        assert (out["dst"] == 7.0).all()
        info = tr.hits_info()
        assert info["calls"] == 0 and info["lastKernelMs"] == 0 and info["totalKernelMs"] == 0 and info["lastMaxHits"] == 0, info
        assert all(np.array_equal(v, tr.stats()[k]) for k, v in stats.items())
        with pytest.raises(rtx.RtError):
            tr.trace_hits(rays[:8], 9)


STATS_MAY_MOVE = ("bvhBuilds", "bvhRebuilds", "bvhRepads")


def test_a_call_moves_no_other_state(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    params, s, t, m = mgr.build_buffers()
    _, _, _, rays = cases("mixed")
    far = rays.copy()
    far["origin"][:16] += np.float32(3e4)                       # (widens the padding)
    want = hc.oracle_hits(rtx, s, t, m, far, 3, hc.BOTH, True, int(params["intersectMode"]))
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
        tb.visibility(rays[:64], 4)
        tb.closest_points(rays[:64])

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "gather_info": tb.gather_info(), "visibility_info": tb.visibility_info(),
                    "closest_info": tb.closest_info(), "stats": tb.stats()}
        before = state()
        assert tb.hits_info()["calls"] == 0
        hc.assert_same_records(rtx, tb.trace_hits(far, 3, True, True), want, "beside an image")
        assert tb.hits_info()["calls"] == 1
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info", "visibility_info", "closest_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            tb.trace_hits(rays[:100], 2)
        assert tb.read_accum().tobytes() == image.tobytes()


def test_manager_raycast_all(rtx):
    mgr = scene_of(rtx, "mesh_test_scene")
    params, s, t, m = mgr.build_buffers()
    rays = hc.batch_of(rtx, s, t, m)[:40]
    with rtx.Tracer(0) as tr:
        mgr.backend = tr
        most = 0
        for i, ray in enumerate(rays):
            for max_hits, both in ((8, True), (2, False)):
                got = mgr.RaycastAll(ray["origin"], ray["direction"], float(ray["tMax"]), max_hits, both)
                want = hc.oracle_hits(rtx, s, t, m, rays[i:i + 1], max_hits, hc.BOTH if both else hc.FRONT, False, int(params["intersectMode"]))[0]
                want = want[want["kind"] != 0]
                assert len(got) == len(want) and (len(got) == 0 or got[0]["hitCount"] == len(got))
                hc.assert_same_records(rtx, got, want, f"RaycastAll ray {i}")
                most = max(most, len(got))
        assert most >= 2                                        # (some ray went through more than one surface)
