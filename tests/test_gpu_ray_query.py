"""Ray queries on the GPU (rt_trace_rays / rt_occluded and their device and rt_multi forms): every field of every rt_hit bitwise against the
CPU oracle's CalculateRayCollision (tests/query_oracle.c), occlusion against the oracle's dst < tMax, on the reference's scenes and on
rays made to hit the edges: random origins inside and outside the scene, unnormalised / axis-aligned / tiny / huge directions, rays that
start on surfaces, NaN / inf origins and zero directions, tMax at the hit distance and one ulp either side, origins far outside the box
padding, both intersect modes, both BVH builders, moving local meshes, and scenes with no triangles or nothing at all.  A query leaves the
renderer's state alone."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from query_check import oracle_hits
from ray_query_helpers import SCENES, camera_rays, make_rays, random_rays, scene_of, shim      # noqa: F401 (shim is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
FLOAT_COLS = [0, 1, 2, 3, 4, 5, 6, 11, 12]          # dst, hitPoint, normal, u, v (the rest are integers)


def assert_hits(got, want, what):
    g, w = got.view(np.uint32).reshape(-1, 16), want.view(np.uint32).reshape(-1, 16)
    same = g == w
    gf, wf = g[:, FLOAT_COLS].view(np.float32), w[:, FLOAT_COLS].view(np.float32)
    same[:, FLOAT_COLS] |= np.isnan(gf) & np.isnan(wf)
    bad = np.where(~same.all(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} hits differ, first {bad[:5].tolist()}:\n got {got[bad[:3]]}\n want {want[bad[:3]]}"


def check_queries(rtx, shim, tracer, spheres, tris, infos, mode, rays, what, mesh_of_chunk=None):
    """closest hit and occlusion of `rays` on `tracer` (which holds the scene) against the oracle; returns the hits"""
    want = oracle_hits(rtx, shim, spheres, tris, infos, mode, rays)
    if mesh_of_chunk is not None:
        tri = want["kind"] == rtx._cabi.RT_HIT_TRIANGLE
        want["mesh"][tri] = np.asarray(mesh_of_chunk)[want["chunk"][tri]]
    got = tracer.trace_rays(rays)
    assert_hits(got, want, what)
    occ = tracer.occluded(rays)
    exp = (want["kind"] != 0).astype(np.uint8)
    bad = np.where(occ != exp)[0]
    assert len(bad) == 0, (f"{what}: occlusion differs on {len(bad)} rays: occluded {occ[bad[:8]].tolist()} where the closest hit's kind is "
                           f"{want['kind'][bad[:8]].tolist()}, first {bad[:8].tolist()}")
    return got


def loaded_tracer(rtx, mgr, mode, **options):
    params, spheres, tris, infos = mgr.build_buffers()
    params["intersectMode"] = mode
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    return t, params, spheres, tris, infos


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", SCENES + ["mesh_test_scene"])
def test_camera_rays_of_the_reference_scenes(rtx, shim, name, mode):
    t, params, s, tr, mi = loaded_tracer(rtx, scene_of(rtx, name), mode)
    with t:
        check_queries(rtx, shim, t, s, tr, mi, mode, camera_rays(rtx, params), f"{name} mode {mode}")


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, shim, compact_nodes):
    """three stack entries per lane in LDS, the rest of the Knight's tree in the global overflow area (both node forms)"""
    t, params, s, tr, mi = loaded_tracer(rtx, scene_of(rtx, "Knight"), 0, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes)
    with t:
        check_queries(rtx, shim, t, s, tr, mi, 0, camera_rays(rtx, params, 48, 32), f"lds_stack 3 compact_nodes {compact_nodes}")
        assert t.stats()["bvhMaxStack"] > 3         # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_random_rays_directions_surfaces_and_special_values(rtx, shim, mode, device_bvh):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, mode, device_bvh=device_bvh)
    with t:
        what = f"mode {mode} device_bvh {device_bvh}"
        rays = random_rays(rtx, tr, s, 4096, seed=11 + mode)
        hits = check_queries(rtx, shim, t, s, tr, mi, mode, rays, "random rays " + what)
        assert (hits["kind"] == 1).any() and (hits["kind"] == 2).any() and (hits["kind"] == 0).any()
        # direction magnitudes: dst is in units of |direction|
        for scale in (1e-8, 1e-3, 1e3, 1e8):
            r = rays.copy()
            r["direction"] *= np.float32(scale)
            check_queries(rtx, shim, t, s, tr, mi, mode, r, f"direction x {scale:g} " + what)
        # rays that start on surfaces: the hit points of the query above, new random directions and the mirrored ones
        hit = hits[hits["kind"] != 0]
        rng = np.random.default_rng(5)
        d = rng.standard_normal((len(hit), 3)).astype(np.float32)
        check_queries(rtx, shim, t, s, tr, mi, mode, make_rays(rtx, hit["hitPoint"], d), "from surfaces " + what)
        nd = np.sum(hit["normal"] * d, 1, keepdims=True)
        check_queries(rtx, shim, t, s, tr, mi, mode, make_rays(rtx, hit["hitPoint"], np.abs(nd) * hit["normal"]), "off surfaces " + what)
        # NaN / inf origins, zero directions
        o = np.asarray(rays["origin"][:64]).copy()
        o[:16, 0], o[16:32, 1], o[32:48, 2] = np.nan, np.inf, -np.inf
        d = np.asarray(rays["direction"][:64]).copy()
        d[48:] = 0.0
        check_queries(rtx, shim, t, s, tr, mi, mode, make_rays(rtx, o, d), "NaN / inf / zero " + what)
        # tMax at the hit distance, one ulp above and below, 0, negative, NaN
        r = rays[hits["kind"] != 0]
        dst = hits["dst"][hits["kind"] != 0]
        for tm, label in ((dst, "dst"), (np.nextafter(dst, np.float32(np.inf)), "dst + 1 ulp"), (np.nextafter(dst, np.float32(0)), "dst - 1 ulp"),
                          (np.float32(0), "0"), (np.float32(-0.0), "-0"), (np.float32(-1), "-1"), (np.float32(np.nan), "NaN")):
            rr = r.copy()
            rr["tMax"] = tm
            got = check_queries(rtx, shim, t, s, tr, mi, mode, rr, f"tMax = {label} " + what)
            if label == "dst + 1 ulp":
                assert (got["kind"] != 0).all()
            if label != "dst + 1 ulp" and label != "dst - 1 ulp":
                assert (got["kind"] == 0).all(), label


def test_far_origins_widen_the_padding(rtx, shim):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0)
    with t:
        near = random_rays(rtx, tr, s, 512, seed=3)
        check_queries(rtx, shim, t, s, tr, mi, 0, near, "near")
        repads = t.stats()["bvhRepads"]
        rng = np.random.default_rng(9)
        centre = np.asarray(tr["posA"]).reshape(-1, 3).mean(0).astype(np.float32)
        dirs = rng.standard_normal((1024, 3)).astype(np.float32)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        o = (centre + 1e5 * dirs).astype(np.float32)
        aim = (centre + rng.standard_normal((1024, 3)).astype(np.float32) * 2) - o
        hits = check_queries(rtx, shim, t, s, tr, mi, 0, make_rays(rtx, o, aim), "origins 1e5 away")
        assert t.stats()["bvhRepads"] > repads
        assert (hits["kind"] != 0).any()


def test_local_meshes_after_new_transforms(rtx, shim):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, spheres, _, _ = mgr.build_buffers()
    ltris, chunks = mgr.build_local_buffers()
    xf = mgr.build_transforms()
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres)
        t.upload_local_meshes(ltris, chunks, len(mgr.meshes))
        t.set_mesh_transforms(xf)
        t.render(0, 1)                                   # built and traced once: the next poses take the geometry pass
        xf2 = xf.copy()
        xf2["position"] += np.float32(0.75)
        xf2["rotation"][:, 1] = np.float32(0.2)
        xf2["rotation"][:, 3] = np.float32(np.sqrt(1 - 0.04))
        t.set_mesh_transforms(xf2)
        world, infos = t.read_world_geometry()
        mesh_of_chunk = chunks["meshIndex"].astype(np.int32)
        for rays, what in ((camera_rays(rtx, params), "camera"), (random_rays(rtx, world, spheres, 2048, seed=21), "random")):
            hits = check_queries(rtx, shim, t, spheres, world, infos, 0, rays, "local meshes, " + what, mesh_of_chunk)
            assert (hits["mesh"][hits["kind"] == 2] >= 0).all()


def far_rays(rtx, tris, n, distance, seed):
    """rays from `distance` away aimed at the scene's centre (+- 2 units)"""
    rng = np.random.default_rng(seed)
    centre = np.asarray(tris["posA"]).reshape(-1, 3).mean(0).astype(np.float32)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o = (centre + np.float32(distance) * dirs).astype(np.float32)
    return make_rays(rtx, o, (centre + rng.standard_normal((n, 3)).astype(np.float32) * 2) - o)


def local_tracer(rtx, mgr, **options):
    """a context holding mgr's meshes through the on-device geometry pipeline, built and traced once, then moved: (tracer, params,
    spheres, world triangles, world chunks, mesh of each chunk)"""
    params, spheres, _, _ = mgr.build_buffers()
    ltris, chunks = mgr.build_local_buffers()
    xf = mgr.build_transforms()
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=spheres)
    t.upload_local_meshes(ltris, chunks, len(mgr.meshes))
    t.set_mesh_transforms(xf)
    t.render(0, 1)
    xf["position"] += np.float32(0.5)
    t.set_mesh_transforms(xf)
    world, infos = t.read_world_geometry()
    return t, params, spheres, world, infos, chunks["meshIndex"].astype(np.int32)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_far_origins_take_the_geometry_pass(rtx, shim, device_bvh):
    """Origins 1e5 away on a local-mesh scene: the padding is widened by a geometry pass with the query's bound (cover_origins ->
    run_geometry_kernels(min_G)); with device_bvh = 1 and rebuild_percent = 1 that pass rebuilds the tree, for the same bound."""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    opts = {"device_bvh": device_bvh, **({"rebuild_percent": 1} if device_bvh else {})}
    t, params, s, world, infos, mesh_of_chunk = local_tracer(rtx, mgr, **opts)
    with t:
        before = t.stats()
        hits = check_queries(rtx, shim, t, s, world, infos, 0, far_rays(rtx, world, 1024, 1e5, seed=9), f"local, 1e5 away, device_bvh {device_bvh}",
                             mesh_of_chunk)
        assert (hits["kind"] == 2).any()
        after = t.stats()
        assert after["lastGeometryMs"] != before["lastGeometryMs"] or after["bvhRebuilds"] > before["bvhRebuilds"]
        if device_bvh:
            assert after["bvhRebuilds"] > before["bvhRebuilds"]
        check_queries(rtx, shim, t, s, world, infos, 0, random_rays(rtx, world, s, 1024, seed=10), "local, near after far", mesh_of_chunk)
        assert t.read_world_geometry()[0].tobytes() == world.tobytes()


def test_origins_beyond_half_the_float_range(rtx, shim):
    """A finite origin above FLT_MAX / 2: the padding is capped at FLT_MAX instead of overflowing to +inf.  The widened boxes prune
    nothing, so every later query is still the oracle's, and the image is the one rendered without the query."""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    ta, params, s, tr, mi = loaded_tracer(rtx, mgr, 0)
    with ta:
        ta.render(0, 4)
        want = ta.read_accum()
    t, *_ = loaded_tracer(rtx, mgr, 0)
    with t:
        t.render(0, 2)
        far = far_rays(rtx, tr, 64, 3e38, seed=12)
        t.trace_rays(far)
        t.occluded(far)
        assert t.stats()["bvhRepads"] >= 1
        check_queries(rtx, shim, t, s, tr, mi, 0, random_rays(rtx, tr, s, 2048, seed=14), "near, after origins at 3e38")
        f32, f16 = t.read_bvh()
        assert not np.isnan(f32.view(np.float32)[:, :24]).any()
        t.render(2, 2)
        assert t.read_accum().tobytes() == want.tobytes()


def test_multi_tracer_on_local_meshes(rtx, shim):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    t, params, s, world, infos, mesh_of_chunk = local_tracer(rtx, mgr)
    rays = np.concatenate([random_rays(rtx, world, s, 3000, seed=15), far_rays(rtx, world, 500, 1e5, seed=16)])
    with t:
        want = check_queries(rtx, shim, t, s, world, infos, 0, rays, "local, one context", mesh_of_chunk)
    xf = mgr.build_transforms()
    xf["position"] += np.float32(0.5)
    with rtx.MultiTracer([0] * 3) as m:
        m.set_params(params)
        m.upload(spheres=s)
        m.upload_local_meshes(*mgr.build_local_buffers(), len(mgr.meshes))
        m.set_mesh_transforms(xf)
        assert m.trace_rays(rays).tobytes() == want.tobytes()
        assert np.array_equal(m.occluded(rays), (want["kind"] != 0).astype(np.uint8))


def test_spheres_only_empty_scene_no_params_and_zero_rays(rtx, shim):
    mgr = scene_of(rtx, "Balls_Outdoors")
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0)
    with t:
        check_queries(rtx, shim, t, s, tr, mi, 0, random_rays(rtx, tr, s, 1024, seed=4), "spheres only")
        assert len(t.trace_rays(np.zeros(0, rtx.RAY))) == 0 and len(t.occluded(np.zeros(0, rtx.RAY))) == 0
    mesh = rtx.scenes.mesh_test_scene(64, 48)
    _, s, tr, mi = mesh.build_buffers()
    with rtx.Tracer(0) as t:                             # no rt_set_params: RT_INTERSECT_FLAT_CHUNKS
        t.upload(spheres=s, triangles=tr, meshinfo=mi)
        check_queries(rtx, shim, t, s, tr, mi, 0, random_rays(rtx, tr, s, 2048, seed=6), "no params")
    with rtx.Tracer(0) as t:                             # nothing uploaded
        rays = random_rays(rtx, tr, s, 256, seed=8)
        got = t.trace_rays(rays)
        assert (got["kind"] == 0).all() and np.isinf(got["dst"]).all() and (got["primitive"] == -1).all()
        assert not t.occluded(rays).any()
        t.upload(spheres=np.zeros(0, rtx.SPHERE), triangles=np.zeros(0, rtx.TRIANGLE), meshinfo=np.zeros(0, rtx.MESHINFO))
        assert (t.trace_rays(rays)["kind"] == 0).all()


def test_error_codes(rtx):
    lib = rtx.load_library()
    rays = np.zeros(4, rtx.RAY)
    hits = np.zeros(4, rtx.HIT)
    occ = np.zeros(4, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert lib.rt_trace_rays(None, p(rays), 4, p(hits)) == -1
    assert lib.rt_occluded_device(None, p(rays), 4, p(occ)) == -1
    assert lib.rt_multi_trace_rays(None, p(rays), 4, p(hits)) == -1
    with rtx.Tracer(0) as t:
        c = t._ctx
        assert lib.rt_trace_rays(c, p(rays), 0, None) == 0 and lib.rt_occluded_device(c, None, 0, None) == 0
        for call, out in ((lib.rt_trace_rays, hits), (lib.rt_occluded, occ), (lib.rt_trace_rays_device, hits), (lib.rt_occluded_device, occ)):
            assert call(c, p(rays), -1, p(out)) == -2
            assert call(c, None, 4, p(out)) == -2 and call(c, p(rays), 4, None) == -2
            assert lib.rt_last_error(c)
        assert lib.rt_trace_rays_device(c, p(rays), 4, p(hits)) == -2          # host memory is not device memory
        assert b"device" in lib.rt_last_error(c)


def test_device_entries_on_tensors_match_the_host_entries():
    """(in a fresh process that imports torch first: tests/ray_query_torch_worker.py)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "ray_query_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device entries ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_multi_tracer_gives_the_single_context_bits(rtx):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    t, params, s, tr, mi = loaded_tracer(rtx, mgr, 0)
    rays = random_rays(rtx, tr, s, 5001, seed=17)
    with t:
        want, want_occ = t.trace_rays(rays), t.occluded(rays)
    with rtx.MultiTracer([0] * 3) as m:
        m.set_params(params)
        m.upload(spheres=s, triangles=tr, meshinfo=mi)
        assert m.trace_rays(rays).tobytes() == want.tobytes()
        assert np.array_equal(m.occluded(rays), want_occ)


STATS_KEPT = ("numRenderedFrames", "rays", "sphereTests", "nodeVisits", "triTests", "hits", "phaseLanes", "phaseExecs", "regionExecs",
              "lastKernelMs", "totalKernelMs", "lastFramesPerLaunch", "lastKernel", "lastFramesInterleaved", "queuedLaunches",
              "primaryListBuilds", "numBvhNodes", "numTriangles")


def test_queries_do_not_disturb_the_render(rtx):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    K = 3
    ta, params, s, tr, mi = loaded_tracer(rtx, mgr, 0)
    with ta:
        ta.render(0, 2 * K)
        want = ta.read_accum()
    tb, *_ = loaded_tracer(rtx, mgr, 0)
    with tb:
        tb.render(0, K)
        before = tb.stats()
        tb.trace_rays(random_rays(rtx, tr, s, 1000, seed=1))
        far = random_rays(rtx, tr, s, 100, seed=2)
        far["origin"] *= np.float32(1e4)                       # widens the padding
        tb.occluded(far)
        tb.trace_rays(far)
        after = tb.stats()
        for k in STATS_KEPT:
            assert before[k] == after[k], k
        assert after["bvhRepads"] > before["bvhRepads"]
        tb.render(K, K)
        got = tb.read_accum()
    assert got.tobytes() == want.tobytes()


def test_manager_raycast_returns_the_component(rtx, shim):
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, tr, mi = mgr.build_buffers()
    with rtx.Tracer(0) as t:
        mgr.backend = t
        pos = np.asarray(params["worldSpaceCameraPos"], np.float32)
        targets = [np.asarray(sp.transform.position, np.float32) for sp in mgr.spheres] + \
                  [np.asarray(m.transform.position, np.float32) for m in mgr.meshes]
        rays = make_rays(rtx, np.broadcast_to(pos, (len(targets), 3)), np.stack(targets) - pos)
        want = oracle_hits(rtx, shim, s, tr, mi, 0, rays)
        chunk_mesh = np.repeat(np.arange(len(mgr.meshes)), [len(m.GetSubMeshes()) for m in mgr.meshes])
        kinds = set()
        for r, w in zip(rays, want):
            hit, comp = mgr.Raycast(r["origin"], r["direction"])
            assert hit.tobytes() == w.tobytes()
            kinds.add(int(w["kind"]))
            if w["kind"] == 1:
                assert comp is mgr.spheres[int(w["primitive"])]
            elif w["kind"] == 2:
                assert comp is mgr.meshes[int(chunk_mesh[int(w["chunk"])])]
            else:
                assert comp is None
        assert {1, 2} <= kinds
        hit, comp = mgr.Raycast(pos, -(targets[0] - pos))          # away from everything ... or not: the answer is the oracle's
        w = oracle_hits(rtx, shim, s, tr, mi, 0, make_rays(rtx, pos[None], -(targets[0] - pos)[None]))[0]
        assert hit.tobytes() == w.tobytes() and (comp is None) == (w["kind"] == 0)


def test_manager_raycast_with_device_geometry(rtx, shim):
    """RayTracingManager.deviceGeometry = True: the mesh comes from the hit's mesh index (the local-mesh upload)"""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, s, _, _ = mgr.build_buffers()
    _, chunks = mgr.build_local_buffers()
    with rtx.Tracer(0) as t:
        mgr.backend, mgr.deviceGeometry = t, True
        pos = np.asarray(params["worldSpaceCameraPos"], np.float32)
        targets = [np.asarray(m.transform.position, np.float32) for m in mgr.meshes] + [np.asarray(sp.transform.position, np.float32) for sp in mgr.spheres]
        got = [mgr.Raycast(pos, tg - pos) for tg in targets]
        world, infos = t.read_world_geometry()
        rays = make_rays(rtx, np.broadcast_to(pos, (len(targets), 3)), np.stack(targets) - pos)
        want = oracle_hits(rtx, shim, s, world, infos, 0, rays)
        tri = want["kind"] == 2
        want["mesh"][tri] = chunks["meshIndex"].astype(np.int32)[want["chunk"][tri]]
        kinds = set()
        for (hit, comp), w in zip(got, want):
            assert hit.tobytes() == w.tobytes()
            kinds.add(int(w["kind"]))
            if w["kind"] == 1:
                assert comp is mgr.spheres[int(w["primitive"])]
            elif w["kind"] == 2:
                assert comp is mgr.meshes[int(w["mesh"])]
            else:
                assert comp is None
        assert 2 in kinds


def device_free_bytes():
    """hipMemGetInfo's free figure, from the HIP runtime the library has loaded (found among this process's mappings)"""
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
    hip = ctypes.CDLL(paths.pop())
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_destroying_a_context_gives_its_query_staging_back(rtx):
    """Six contexts in turn each make one host-entry radiance, SH9 gather and SH9 visibility call on 2^18 points and are closed.  Their
    results are staged in 2^18 * (16 + 144 + 48) B = 54.5 MB a round.  The device's free memory after the sixth close may not lie below
    the figure after the first by more than that one round; contexts that kept their staging past rt_destroy would be five rounds, 272 MB,
    down.  (Free memory is device-wide: more rounds, not a wider bound, if other users of the device ever move it by tens of MB.)"""
    n, rounds = 1 << 18, 6
    one_round = n * (16 + 144 + 48)
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, spheres, tris, infos = mgr.build_buffers()
    rng = np.random.default_rng(11)
    normals = rng.standard_normal((n, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    points = make_rays(rtx, rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32), normals)
    free = []
    for _ in range(rounds):
        with rtx.Tracer(0) as t:
            t.set_params(params)
            t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
            assert t.trace_radiance(points, samples=1).shape == (n, 4)
            assert t.gather(points, samples=1, mode=rtx._cabi.GATHER_SH9).shape == (n, 9, 4)
            assert t.visibility(points, samples=1, mode=rtx._cabi.VIS_SH9).shape == (n, 12)
        free.append(device_free_bytes())
    print(f"free after each close: {free}; after round 1 - after round {rounds} = {free[0] - free[-1]} B, bound {one_round} B")
    assert free[0] - free[-1] <= one_round, (f"free memory fell by {free[0] - free[-1]} B between the first and the last of {rounds} closed contexts "
                                              f"(bound: one round's staging, {one_round} B): {free}")
