"""The four query families (rt_trace_rays / rt_occluded, rt_trace_radiance, rt_gather, rt_visibility, their device entries and their
rt_multi forms) on the renderer fuzz's scenes (test_gpu_fuzz.random_scene: duplicate and coplanar stacks, integer-grid quads, slivers,
zero-area, NaN, infinite and 3e37-sized triangles, loose and cut chunk boxes, permuted AllMeshInfo, zero-radius spheres, the scene 1e5
units away, the far mirror sphere), with the items and the knob draw of tests/query_fuzz.py: rays through shared edges and corners, bounds
at a hit's distance and one ulp either side, surface points, special directions and a degenerate handful; builder options, lds_stack, the
three slice sizes, the sample count, the stream seed, a wrapping firstIndex and the intersect mode drawn together.  Every family equals
its CPU checker bit for bit, the families agree with each other where they must, the device entries equal the host entries, and an
rt_multi of three contexts gives the single context's bits.  The two per-lane families that came later, rt_trace_hits and
rt_closest_points, have a test of their own on the same scenes and builder options: the items as rays in a drawn (K, sides, countAll)
form and as the whole eight-record list, and points of their own (qf.fuzz_points: on shared corners and triplicated triangles, at a
hit's distance and one ulp either side of it as the radius, far outside, radii whose square overflows or underflows), every word of
every record against hits_check and closest_check, and against rt_trace_rays / rt_occluded where the definitions meet.
RTX_FUZZ_SEEDS / RTX_FUZZ_FIRST choose the seeds, as for test_gpu_fuzz.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
import hits_check as hc
import query_check as gc
import query_fuzz as qf
import query_check as vc
from query_check import oracle_candidates, oracle_hits
from ray_query_helpers import camera_rays, make_rays, shim      # noqa: F401 (shim is a fixture)
from test_gpu_ray_query import FLOAT_COLS, check_queries

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_FIRST = int(os.environ.get("RTX_FUZZ_FIRST", "0"))
_SEEDS = int(os.environ.get("RTX_FUZZ_SEEDS", "24"))       # RTX_FUZZ_SEEDS=400 [RTX_FUZZ_FIRST=300] for a soak run
HIT_WORDS = ("dst", "hitPoint.x", "hitPoint.y", "hitPoint.z", "normal.x", "normal.y", "normal.z", "kind", "primitive", "chunk", "mesh", "u", "v",
             "word 13", "word 14", "word 15")


def same_hits(got, want, items, what):
    g, w = got.view(np.uint32).reshape(-1, 16), want.view(np.uint32).reshape(-1, 16)
    same = g == w
    gf, wf = g[:, FLOAT_COLS].view(np.float32), w[:, FLOAT_COLS].view(np.float32)
    same[:, FLOAT_COLS] |= np.isnan(gf) & np.isnan(wf)
    bad = np.where(~same.all(1))[0]
    if len(bad):
        i = bad[0]
        words = [HIT_WORDS[k] for k in np.where(~same[i])[0]]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} hits differ, first {qf.describe(items, i)}: words {words}\n got  {got[i]}\n want {want[i]}")


def same_bits(got, want, items, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
    same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == np.float32 else g == w
    if g.dtype == np.float32:
        same = same | (np.isnan(g) & np.isnan(w))
    bad = np.where(~same.all(1))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} items differ, first {qf.describe(items, i)}:\n got  {g[i].tolist()}\n want {w[i].tolist()}")


@pytest.fixture(scope="module")
def device_entries():
    """seed -> None or what differed: tests/query_fuzz_torch_worker.py, once for all seeds, in a fresh process"""
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "query_fuzz_torch_worker.py"), str(_FIRST), str(_SEEDS)],
                           capture_output=True, text=True, timeout=120 + _SEEDS)      # (measured: 4.6 s for 24 seeds, 24.9 s for 400; with rt_trace_hits and rt_closest_points in it 5.2 s for 24, 21.3 s for 200)
        out, err, rc = r.stdout, r.stderr, r.returncode
    except subprocess.TimeoutExpired as e:
        out, err, rc = (e.stdout or b"").decode(errors="replace"), (e.stderr or b"").decode(errors="replace"), "timeout"
    lines = [line for line in out.splitlines() if line.startswith("QUERY_FUZZ_DEVICE ")]
    reached = [line for line in out.splitlines() if line.startswith("QUERY_FUZZ_SEED ")]
    assert rc == 0 and lines, f"the device-entry worker ended with {rc}; the last seed it started: {reached[-1:]}\n{out[-2000:]}{err[-4000:]}"
    return {int(k): v for k, v in json.loads(lines[-1][len("QUERY_FUZZ_DEVICE "):]).items()}


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _SEEDS))
def test_query_families_on_a_random_scene(rtx, shim, device_entries, seed):
    scene, items, options, call = qf.fuzz_case(rtx, seed, shim)
    p, sph, tris, infos = scene
    mode = int(p["intersectMode"])
    N, s, f = call["samples"], call["seed"], call["first_index"]
    ctx = f"fuzz seed {seed} ({len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres), options {options}, call {call}"
    with np.errstate(invalid="ignore"):
        traced = items["tMax"] > 0
    t = rtx.Tracer(0)                                    # a context of its own: the options include the builder's
    try:
        qf.load_scene(t, scene, options)
        # ---- ray queries: every word of every hit, and occlusion = the checker's t < inf
        want = oracle_hits(rtx, shim, sph, tris, infos, mode, items)
        hits = t.trace_rays(items)
        same_hits(hits, want, items, "trace_rays, " + ctx)
        occ = t.occluded(items)
        same_bits(occ, (want["dst"] < np.inf).astype(np.uint8), items, "occluded, " + ctx)
        # ---- the sampled families against their checkers
        got = {}
        for family, fmode in qf.FAMILIES:
            got[family, fmode] = qf.run_family(t, items, call, family, fmode)
            same_bits(got[family, fmode], qf.checker(rtx, scene, items, call, family, fmode), items, f"{family} mode {fmode}, " + ctx)
        assert device_entries[seed] is None, device_entries[seed]
        # ---- visibility mode 0's open count = the zeros of rt_occluded over the point's drawn directions and reach
        rays = vc.sample_rays(rtx, items, N, s, f, vc.COSINE)
        blocked = np.asarray(t.occluded(rays)).reshape(len(items), N).astype(np.int64)
        open_ = np.where(traced, N - blocked.sum(1), 0)
        same_bits(got["visibility", vc.COSINE][:, 3], (open_.astype(np.float32) / np.float32(N)).astype(np.float32), items,
                  "visibility mode 0's fraction against rt_occluded, " + ctx)
        assert (blocked[~traced] == 0).all()
        # ---- gather with one sample = the radiance query along that one direction
        d = gc.directions(rtx, items, 0, s, f, gc.COSINE)
        same_bits(t.gather(items, 1, s, f, gc.COSINE), t.trace_radiance(make_rays(rtx, items["origin"], d, items["tMax"]), 1, s, f), items,
                  "gather N = 1 against trace_radiance, " + ctx)
        # ---- through an rt_multi of three contexts on the device: the split with the slices and the wrapping firstIndex
        if seed % 3 == 0:
            with rtx.MultiTracer([0] * 3) as m:
                qf.load_scene(m, scene, options)
                same_hits(m.trace_rays(items), hits, items, "rt_multi trace_rays, " + ctx)
                same_bits(m.occluded(items), occ, items, "rt_multi occluded, " + ctx)
                for family, fmode in qf.FAMILIES:
                    same_bits(qf.run_family(m, items, call, family, fmode), got[family, fmode], items, f"rt_multi {family} mode {fmode}, " + ctx)
    finally:
        t.close()


SHARED = ("dst", "hitPoint", "normal", "kind", "primitive", "chunk", "mesh", "u", "v")      # of a ray-query hit and a multi-hit record


def same_records(check, rtx, got, want, items, what):
    """check.assert_same_records (hits_check's or closest_check's: every word of every record), its message naming the first item whose
    records differ in any bit"""
    g, w = (np.ascontiguousarray(a).reshape(len(items), -1).view(np.uint32) for a in (got, want))
    differ = np.flatnonzero((g != w).any(1)) if g.shape == w.shape else []
    check.assert_same_records(rtx, got, want, what + (f"; first {qf.describe(items, differ[0])}" if len(differ) else ""))


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _SEEDS))
def test_point_and_multihit_queries_on_a_random_scene(rtx, shim, device_entries, seed):
    """rt_trace_hits on the items and rt_closest_points on qf.fuzz_points, on the same scenes and builder options, with slices and a
    multi-hit form of their own draw (qf.point_knobs)"""
    scene, items, options, _ = qf.fuzz_case(rtx, seed, shim)
    p, sph, tris, infos = scene
    more, form = qf.point_knobs(seed)
    options = {**options, **more}
    points = qf.fuzz_points(rtx, seed, scene, items, shim)
    mode = int(p["intersectMode"])
    ctx = f"fuzz seed {seed} ({len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres), options {options}, intersectMode {mode}"
    t = rtx.Tracer(0)                                    # a context of its own: the options include the builder's
    try:
        qf.load_scene(t, scene, options)
        # ---- multi-hit queries: the drawn form and the whole list (eight records, both sides, every hit counted) against the checker
        got = {}
        for name, f in (("drawn", form), ("deep", qf.DEEP)):
            got[name] = qf.run_hits(t, items, f)
            same_records(hc, rtx, got[name], qf.check_hits(rtx, scene, items, f), items, f"trace_hits {f}, " + ctx)
        # ---- ... against the device's own ray queries: record 0, front faces, is rt_trace_rays' hit where that hit is untied (at a
        # tie the two entries keep different candidates by definition), and a hit is there when rt_occluded says so, on every ray
        first = t.trace_hits(items, 1)[:, 0]
        hits, occ = t.trace_rays(items), t.occluded(items)
        clear = np.flatnonzero(oracle_candidates(rtx, shim, sph, tris, infos, mode, items) < 2)
        for f in SHARED:
            a, b = first[f][clear].reshape(len(clear), -1), hits[f][clear].reshape(len(clear), -1)
            same = a.view(np.uint32) == b.view(np.uint32)
            if a.dtype == np.float32:
                same |= np.isnan(a) & np.isnan(b)
            bad = clear[~same.all(1)]
            assert not len(bad), f"trace_hits K = 1 against trace_rays, {f}, {ctx}: {len(bad)} rays differ, first {qf.describe(items, bad[0])}:\n got  {first[bad[0]]}\n want {hits[bad[0]]}"
        same_bits(first["hitCount"].astype(np.uint8), occ, items, "trace_hits K = 1 hitCount against occluded, " + ctx)
        # ---- ... and against itself: K records are the first K of eight
        for both, count_all in ((0, 0), (1, 1)):
            f8 = {"K": 8, "both_sides": both, "count_all": count_all}
            deep = got["deep"] if f8 == qf.DEEP else qf.run_hits(t, items, f8)
            for K in (1, 2, 3):
                want = deep[:, :K].copy()
                if not count_all:
                    want["hitCount"] = np.minimum(want["hitCount"], K)
                same_records(hc, rtx, qf.run_hits(t, items, {**f8, "K": K}), want, items, f"trace_hits K = {K} against the first {K} of {f8}, " + ctx)
        # ---- closest-point queries against the checker
        near = t.closest_points(points)
        same_records(cc, rtx, near, cc.oracle_closest(rtx, sph, tris, infos, points), points, "closest_points, " + ctx)
        assert device_entries[seed] is None, device_entries[seed]
        # ---- through an rt_multi of three contexts on the device
        if seed % 3 == 0:
            with rtx.MultiTracer([0] * 3) as m:
                qf.load_scene(m, scene, options)
                for name, f in (("drawn", form), ("deep", qf.DEEP)):
                    same_records(hc, rtx, qf.run_hits(m, items, f), got[name], items, f"rt_multi trace_hits {f}, " + ctx)
                same_records(cc, rtx, m.closest_points(points), near, points, "rt_multi closest_points, " + ctx)
    finally:
        t.close()


def test_coinciding_local_meshes_hit_the_first_in_list_order(rtx, shim):
    """Two pairs of local meshes refitted onto the same transform: their triangles coincide, every hit on them has a second candidate at
    the same dst, and prim, chunk and mesh are those of the mesh that comes first in the list"""
    mgr = rtx.scenes.mesh_test_scene(64, 48)
    params, spheres, _, _ = mgr.build_buffers()
    ltris, chunks = mgr.build_local_buffers()
    xf = mgr.build_transforms()
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres)
        t.upload_local_meshes(ltris, chunks, len(mgr.meshes))
        t.set_mesh_transforms(xf)
        t.render(0, 1)                                   # built and traced once: the next poses are a refit
        xf2 = xf.copy()
        xf2[4], xf2[5] = xf2[2], xf2[3]                  # the second cube onto the first, the second ball onto the first
        t.set_mesh_transforms(xf2)
        world, infos = t.read_world_geometry()
        mesh_of_chunk = chunks["meshIndex"].astype(np.int32)
        pos = np.asarray(params["worldSpaceCameraPos"], np.float32)
        twice = np.isin(mesh_of_chunk, (2, 3))
        centroids = np.concatenate([(world["posA"] + world["posB"] + world["posC"])[int(c["firstTriangleIndex"]):int(c["firstTriangleIndex"]) + int(c["numTriangles"])]
                                    for c in chunks[twice]]) / np.float32(3)
        rays = np.concatenate([camera_rays(rtx, params), make_rays(rtx, np.broadcast_to(pos, centroids.shape), centroids - pos)])
        hits = check_queries(rtx, shim, t, spheres, world, infos, 0, rays, "coinciding local meshes", mesh_of_chunk)
        tied = oracle_candidates(rtx, shim, spheres, world, infos, 0, rays) >= 2
        assert tied.sum() >= 100 and np.isin(hits["mesh"][tied], (2, 3)).all(), (int(tied.sum()), np.unique(hits["mesh"][tied]))
        assert not np.isin(hits["mesh"], (4, 5)).any()
