"""Sphere casts on the GPU (option "sweep" = 1 on rt_trace_rays / rt_occluded, their device and rt_multi forms; sweep.py): every field
of every record bit for bit against the brute-force checker (tests/sweep_oracle.c, pinned by tests/test_sweep_cpu.py), on
test_gpu_closest.py's scenes with the batch of sweep_check.batch_of: rays aimed at vertices, edge midpoints and centroids, rays
parallel to edges at offset r (the edge quadratic's cancellation case), balls that start overlapping, rays from 1e4 extents away and
six that are not traced.  Both node forms, both builders, every leaf size, coordinates far from the origin, a traversal stack that
spills, a refitted local-mesh scene, batches cut into two calls and rt_multi, the device entry; the option's refusal; what the option leaves
alone at 0; the state a call leaves alone; and the physical invariant through rt_closest_points."""
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
import sweep_check as sc
from ray_query_helpers import scene_of
from test_gpu_closest import STATS_MAY_MOVE, buffers_of, tracer_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("one", "two", "plane", "spheres", "mixed", "Knight")


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, rays, the checker's records, its occlusion bytes), each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            rays, _ = sc.batch_of(rtx, s, t, m)
            want, occ = sc.oracle_cast(rtx, s, t, m, rays)
            for a in (rays, want, occ):
                a.setflags(write=False)
            cache[name] = (s, t, m, rays, want, occ)
        return cache[name]
    return get


def cast(rtx, tr, rays):
    return rtx.sweep.sphere_cast(tr, rays, sc.radii_of(rays))


def check_batch(rtx, tr, s, t, m, rays, want, occ, what):
    got = cast(rtx, tr, rays)
    sc.assert_same_records(rtx, got, want, what)
    assert (got["kind"][-sc.N_UNTRACED:] == 0).all() and np.isposinf(got["dst"][-sc.N_UNTRACED:]).all()
    chk = rtx.sweep.sphere_check(tr, rays, sc.radii_of(rays))
    assert chk.dtype == np.uint8 and np.array_equal(chk, occ) and np.array_equal(chk, (want["kind"] != 0).astype(np.uint8)), what
    # tMax at the median dst: the hits beyond it turn into misses, the others keep their bits
    q = rays.copy()
    q["tMax"][:-sc.N_UNTRACED] = np.median(want["dst"][np.isfinite(want["dst"])])
    wq, oq = sc.oracle_cast(rtx, s, t, m, q)
    assert 0 < (wq["kind"] != 0).sum() < (want["kind"] != 0).sum()
    sc.assert_same_records(rtx, cast(rtx, tr, q), wq, what + ", tMax = the median dst")
    assert np.array_equal(rtx.sweep.sphere_check(tr, q, sc.radii_of(q)), oq), what


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, rays, want, occ = cases(name)
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_batch(rtx, tr, s, t, m, rays, want, occ, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("plane", "Knight"):
        s, t, m, rays, want, _ = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            sc.assert_same_records(rtx, cast(rtx, tr, rays), want, f"{name} max_leaf {max_leaf}")


@pytest.mark.parametrize("name", ["two", "mixed", "Knight"])
def test_scene_and_rays_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): the balls stay small while coordinates are large"""
    s, t, m, rays, _, _ = cases(name)
    off = np.array([1e4, -1e4, 1e4], np.float32)
    s2, t2, m2, r2 = s.copy(), t.copy(), m.copy(), rays.copy()
    s2["position"] += off
    for k in ("posA", "posB", "posC"):
        t2[k] += off
    m2["boundsMin"] += off
    m2["boundsMax"] += off
    r2["origin"] += off
    want, occ = sc.oracle_cast(rtx, s2, t2, m2, r2)
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            sc.assert_same_records(rtx, cast(rtx, tr, r2), want, f"{name} translated, compact_nodes {compact_nodes}")
            assert np.array_equal(rtx.sweep.sphere_check(tr, r2, sc.radii_of(r2)), occ)


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, rays, want, occ = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        sc.assert_same_records(rtx, cast(rtx, tr, rays), want, f"lds_stack 3, compact_nodes {compact_nodes}")
        assert np.array_equal(rtx.sweep.sphere_check(tr, rays, sc.radii_of(rays)), occ)
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        rays, _ = sc.batch_of(rtx, s, world, infos, seed=5)
        got = cast(rtx, tr, rays)
        sc.assert_same_records(rtx, got, sc.oracle_cast(rtx, s, world, infos, rays, chunk_mesh)[0], f"local meshes, device_bvh {device_bvh}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_cut_batches_and_the_options_refusal(rtx, cases):
    s, t, m, rays, want, _ = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        for cut in (1, 333):
            sc.assert_same_records(rtx, np.concatenate([cast(rtx, tr, rays[:cut]), cast(rtx, tr, rays[cut:])]), want, f"cut at {cut}")
        lib = rtx.load_library()
        assert lib.rt_set_option(tr._ctx, b"sweep", 2) == -2 and b"sweep" in lib.rt_last_error(tr._ctx)
        assert lib.rt_set_option(tr._ctx, b"sweep", -1) == -2
        sc.assert_same_records(rtx, cast(rtx, tr, rays), want, "after the refusals")
    # the library's own slices (the ray queries': 2^22 rays) cannot be set; a batch longer than one block and a cut inside a wave are
    # what the launch shape can get wrong
    with tracer_of(rtx, s, t, m) as tr:
        sc.assert_same_records(rtx, cast(rtx, tr, rays[:100]), want[:100], "100 rays")


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, rays, want, occ = cases("mixed")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        sc.assert_same_records(rtx, cast(rtx, mt, rays), want, "two contexts")
        assert np.array_equal(rtx.sweep.sphere_check(mt, rays, sc.radii_of(rays)), occ)
        sc.assert_same_records(rtx, cast(rtx, mt, rays[:1]), want[:1], "fewer rays than contexts")


def test_device_entry_on_tensors_matches_the_host_entry():
    """(in a fresh process that imports torch first: tests/sweep_torch_worker.py cast)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "sweep_torch_worker.py"), "cast"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_with_the_option_at_0_the_ray_queries_keep_their_bits(rtx, cases):
    """before and after sphere casts, on rays whose reserved word holds radii, and garbage"""
    s, t, m, rays, want, _ = cases("mixed")
    junk = rays.copy()
    junk["_reserved"][::2] = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31 - 1, len(junk[::2]))
    clean = rays.copy()
    clean["_reserved"] = 0
    with tracer_of(rtx, s, t, m) as tr:
        before = (tr.trace_rays(clean), tr.occluded(clean), tr.trace_hits(clean, 4, both_sides=True))
        sc.assert_same_records(rtx, cast(rtx, tr, rays), want, "the cast in between")
        for r in (clean, rays, junk):
            after = (tr.trace_rays(r), tr.occluded(r), tr.trace_hits(r, 4, both_sides=True))
            for a, b in zip(before, after):
                assert a.tobytes() == b.tobytes()
        assert (before[0]["_reserved"] == 0).all() and (before[0]["kind"] != 0).any()
        # the calls that ignore the option ignore it at 1 as well
        tr.set_option("sweep", 1)
        assert tr.trace_hits(junk, 4, both_sides=True).tobytes() == before[2].tobytes()
        p = cc.points_of(rtx, rays["origin"][:64], 1.0)
        at1 = tr.closest_points(p)
        tr.set_option("sweep", 0)
        assert tr.closest_points(p).tobytes() == at1.tobytes()
    # ... and so do the sampled families and the frames: launch_rays is the one place that reads it
    params, s2, t2, m2 = scene_of(rtx, "mesh_test_scene").build_buffers()
    pts = junk[:64].copy()
    pts["tMax"] = 2.0
    out = {}
    for sweep in (0, 1):
        with rtx.Tracer(0) as tr:
            tr.set_option("sweep", sweep)
            tr.set_params(params)
            tr.upload(spheres=s2, triangles=t2, meshinfo=m2)
            tr.render(0, 2)
            out[sweep] = (tr.read_accum(), tr.visibility(pts, 4), tr.gather(pts, 4), tr.trace_radiance(pts, 4))
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()


def test_a_call_moves_no_other_state(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    params, s, t, m = mgr.build_buffers()
    _, _, _, rays, want, _ = cases("mixed")
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
        sc.assert_same_records(rtx, cast(rtx, tb, rays), want, "beside an image")       # (the far rays widen the padding)
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info", "visibility_info", "closest_info", "hits_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        assert after["stats"]["bvhRepads"] > before["stats"]["bvhRepads"]
        # interleaved with queued frames: the call settles the queue, the frames land as if nothing had been asked in between
        for f in range(K, 2 * K):
            tb.submit_frame(f)
            cast(rtx, tb, rays[:100])
        assert tb.read_accum().tobytes() == image.tobytes()


def test_manager_method(rtx, cases):
    mgr = scene_of(rtx, "mesh_test_scene")
    _, _, _, rays, want, _ = cases("mixed")
    with rtx.Tracer(0) as tr:
        mgr.backend = tr
        sc.assert_same_records(rtx, mgr.SphereCast(rays, sc.radii_of(rays)), want, "RayTracingManager.SphereCast")


M_FREE = 4 * 0.0055         # profiles/sweep_twin_error.txt: the largest 1 - distance / r over free starts, four seeds; fourfold margin


@pytest.mark.parametrize("name", ["one", "plane", "mixed", "Knight", "spheres"])
def test_the_ball_at_the_contact_touches_the_scene(rtx, cases, name):
    """The physical invariant through the existing call: at o + d * dst the scene is r away, within [r (1 - m), g].
    Upper side.  A triangle contact is at most g away by the guard — exactly, because rt_closest_points forms the guard's key.  A scene
    sphere has no guard; its distance carries the rounding of RaySphere's root, about 2^-25 (|o - s| / (R + r))^2 (R + r) (DESIGN.md
    "Sphere casts"): at most 1.0016 r over the batches of four seeds, asserted with a fourfold margin on the excess, 1.0065 r — below g.
    The rays from 1e4 extents away are held to the triangle side only: their sphere roots are off by whole radii, as rt_trace_rays' are.
    Lower side.  Asserted where it means something: on the aimed and the tangent rays that start free — farther than g from every
    surface and outside every sphere (a ball inside a sphere reports nothing of it, by the definition).  A ball that starts overlapping
    travels inside geometry by definition; for that class only the upper side holds, and it is asserted for it as for the others."""
    s, t, m, rays, want, _ = cases(name)
    cls = sc.batch_of(rtx, s, t, m)[1]
    with tracer_of(rtx, s, t, m) as tr:
        got = cast(rtx, tr, rays)
        hit = got["kind"] != 0
        r = sc.radii_of(rays)
        centre = rays["origin"] + rays["direction"] * np.where(hit, got["dst"], 0)[:, None]      # (float32, as the kernel forms it)
        near = tr.closest_points(cc.points_of(rtx, centre))["dst"]
        start = tr.closest_points(cc.points_of(rtx, rays["origin"]))["dst"]
        g = r * sc.GUARD
        inside = np.zeros(len(rays), bool)
        if len(s):
            away = np.linalg.norm(rays["origin"][:, None, :].astype(np.float64) - s["position"][None].astype(np.float64), axis=2)
            inside = (away <= s["radius"][None] + g[:, None]).any(1)
        tri = hit & (got["kind"] == 2)
        sph = hit & (got["kind"] == 1) & (cls != 3)
        free = hit & (cls <= 1) & (start > g) & ~inside
        print(f"{name}: distance / r at a triangle contact <= {(near[tri] / r[tri]).max() if tri.any() else 0:.6f}, at a sphere contact <= "
              f"{(near[sph] / r[sph]).max() if sph.any() else 0:.6f}, over {int(free.sum())} free starts >= {(near[free] / r[free]).min() if free.any() else 1:.6f}")
        assert (near[tri] <= np.sqrt(g[tri] * g[tri])).all()
        assert (near[sph] <= r[sph] * np.float32(1.0065)).all()
        assert free.sum() > 50 and (near[free] >= r[free] * np.float32(1.0 - M_FREE)).all()
