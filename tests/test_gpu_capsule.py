"""Capsule overlap queries on the GPU (rt_closest_points and its device and rt_multi forms with the option "closest_capsule"): every word
of every record — _reserved[1], the bits of s, included — bit for bit against the brute-force checker (tests/capsule_oracle.c, pinned by
tests/test_capsule_cpu.py).  Scenes: one triangle, two that share an edge, a cube, a sphere beside a triangle, a sphere around P0, a
plane of 128 triangles and a mesh of a few hundred for the tree; capsule_check.batch_of's segments (axis-aligned, diagonal, of length
0, 10^3 times longer than the scene, piercing, parallel, beside an edge, over a vertex, along an edge, through and inside spheres, not
searched) in the forms (K, all) of capsule_check.FORMS; batches of 1, 63, 64, 65 and 257; both node forms, both builders, every leaf
size, a spilling stack, a refitted local mesh; far geometry and the two-endpoint rule; cut batches, slices, rt_multi, the device entry;
the options' refusals and the bytes of the other calls before and after."""
import os
import subprocess
import sys

import numpy as np
import pytest

import capsule_check as kc
import closest_check as cc
import nearest_check as nc
import overlap_check as oc
from listed_gpu import ask, check_a_call_moves_no_other_state, check_forms, check_split_calls_and_counting, make_cases
from ray_query_helpers import scene_of
from test_gpu_closest import batch_of, buffers_of, plane, tracer_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("one", "two", "cube", "beside", "around", "plane", "mixed")


def cube(rtx):
    """the cube [0, 2]^3 as 12 triangles, one chunk, outward windings"""
    v = np.array([(x, y, z) for z in (0, 2) for y in (0, 2) for x in (0, 2)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.zeros(12, rtx.TRIANGLE)
    for i, (a, b, c, d) in enumerate(quads):
        for j, (p, q, r) in enumerate(((a, b, c), (a, c, d))):
            t["posA"][2 * i + j], t["posB"][2 * i + j], t["posC"][2 * i + j] = v[p], v[q], v[r]
            n = np.cross(v[q] - v[p], v[r] - v[p])
            t["normalA"][2 * i + j] = t["normalB"][2 * i + j] = t["normalC"][2 * i + j] = n / np.linalg.norm(n)
    m = np.zeros(1, rtx.MESHINFO)
    m["numTriangles"] = 12
    m["boundsMin"], m["boundsMax"] = (0, 0, 0), (2, 2, 2)
    return np.zeros(0, rtx.SPHERE), t, m


def scene(rtx, name):
    if name == "cube":
        return cube(rtx)
    if name in ("beside", "around"):
        _, t, m = buffers_of(rtx, "one")
        s = np.zeros(1, rtx.SPHERE)
        # beside: a ball next to the triangle; around: a ball that holds the whole triangle and every P0 of the batch's grid
        s["position"], s["radius"] = ((6, 1, 0.5), 1.25) if name == "beside" else ((2, 2, 0), 16.0)
        return s, t, m
    return buffers_of(rtx, name)


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, segments, {(K, all): the checker's answer}), each computed once"""
    return make_cases(rtx, "capsule", scene)


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, g, want = cases(name)
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_forms(rtx, tr, "capsule", g, want, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")
        if name == "plane":
            assert tr.stats()["numBvhNodes"] > 5                # (several levels)
    found = kc.counts(want[3, 1])[:, 0]
    assert (found > 0).sum() > len(g) // 8 and (found == 0).sum() >= 8, name
    if name == "around":                                        # inside the solid ball: key 0, side -1
        inside = want[1, 0][:, 0]
        inside = inside[(inside["kind"] == 1) & (inside["dst"] == 0)]
        assert len(inside) > 40 and (inside["side"] == -1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_at_the_wave_and_block_edges(rtx, cases, n):
    s, t, m, g, want = cases("mixed")
    first = 520                                                 # (past the grid: the segments built on triangles and spheres)
    with tracer_of(rtx, s, t, m) as tr:
        for counting in (0, 1):
            tr.set_option("closest_count", counting)
            check_forms(rtx, tr, "capsule", g[first:first + n], {f: w[first:first + n] for f, w in want.items()}, f"{n} segments, closest_count {counting}",
                        [(1, 0), (8, 0), (3, 1)])


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    for name in ("cube", "plane", "mixed"):
        s, t, m, g, want = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            check_forms(rtx, tr, "capsule", g, want, f"{name} max_leaf {max_leaf}", [(8, 0), (1, 1)])


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, g, want = cases("mixed")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        check_forms(rtx, tr, "capsule", g, want, f"lds_stack 3, compact_nodes {compact_nodes}", [(8, 0), (3, 1)])
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        g = kc.batch_of(rtx, s, world, infos, batch_of(rtx, s, world, infos, seed=5))
        for f in ((8, 0), (3, 1)):
            got = ask(tr, "capsule", g, *f)
            kc.assert_same_records(rtx, got, kc.oracle_capsule(rtx, s, world, infos, g, *f, chunk_mesh=chunk_mesh), f"local meshes, device_bvh {device_bvh}, {f}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


@pytest.mark.parametrize("name", ["two", "mixed"])
def test_scene_and_segments_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): the segments stay small while coordinates are large"""
    s, t, m, g, _ = cases(name)
    off = np.array([1e4, -1e4, 1e4], np.float32)
    s2, t2, m2, g2 = s.copy(), t.copy(), m.copy(), g.copy()
    s2["position"] += off
    for k in ("posA", "posB", "posC"):
        t2[k] += off
    m2["boundsMin"] += off
    m2["boundsMax"] += off
    g2["origin"] += off
    want = {f: kc.oracle_capsule(rtx, s2, t2, m2, g2, *f) for f in ((8, 0), (3, 1))}
    assert (kc.counts(want[3, 1])[:, 0] > 0).sum() > 100
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            check_forms(rtx, tr, "capsule", g2, want, f"{name} translated, compact_nodes {compact_nodes}", list(want))


def test_the_origin_bound_sees_both_endpoints(rtx, cases):
    """P0 near the origin, P1 1e4 away: the padding is widened for P1 (one re-padding), and not again for a batch inside that bound; with
    the option at 0 the same inputs are points near the origin and widen nothing"""
    s, t, m, _, _ = cases("cube")
    rng = np.random.default_rng(9)
    p0 = rng.uniform(0.25, 1.75, (130, 3)).astype(np.float32)       # (inside the cube: no P0 passes the scene's own magnitude, 2)
    d = np.zeros((130, 3), np.float32)
    d[:, 0] = 1e4
    d[::2] *= -1
    d[::3, 1] = 7e3
    far = kc.segments_of(rtx, p0, d=d, radius=2.0)
    assert kc.origin_bound(rtx, far) > 9e3 and kc.origin_bound(rtx, far, kc.BOUND_FROM_P0) < 4
    with tracer_of(rtx, s, t, m) as tr:
        before = tr.stats()["bvhRepads"]
        tr.closest_points(far)                                  # as points: P0 alone
        assert tr.stats()["bvhRepads"] == before
        for f in ((8, 0), (3, 1)):
            kc.assert_same_records(rtx, ask(tr, "capsule", far, *f), kc.oracle_capsule(rtx, s, t, m, far, *f), f"P1 far away, {f}")
        assert tr.stats()["bvhRepads"] == before + 1
        ask(tr, "capsule", far[:7], 2, 0)
        assert tr.stats()["bvhRepads"] == before + 1
        # P0 and d finite, P0 + d = +inf: not searched
        over = kc.segments_of(rtx, [(3e38, 0, 0), (1, 1, 1)], d=[(3e38, 0, 0), (0, 0, 1)], radius=np.inf)
        kc.assert_same_records(rtx, ask(tr, "capsule", over, 2, 1), kc.oracle_capsule(rtx, s, t, m, over, 2, 1), "P1 overflows")


def test_slices_split_calls_and_counting(rtx, cases):
    s, t, m, g, want = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        tr.set_option("closest_slice", 1)
        check_forms(rtx, tr, "capsule", g[500:560], {f: w[500:560] for f, w in want.items()}, "closest_slice 1", [(2, 0), (3, 1)])
        tr.set_option("closest_slice", 100)
        check_forms(rtx, tr, "capsule", g, want, "closest_slice 100", [(8, 0)])
        # counts: one sphere or triangle examined is one test; never more than brute force, and exactly brute force with R = +inf and all = 1
        live = int(sum(i["numTriangles"] for i in m)) + len(s)
        searched = int(kc.searched(g).sum())

        def unbounded_is_brute_force():
            u = _unbounded(g)
            kc.assert_same_records(rtx, ask(tr, "capsule", u, 1, 1), kc.oracle_capsule(rtx, s, t, m, u, 1, 1), "unbounded, all")
            assert tr.closest_info()["lastPrimTests"] == searched * live, (tr.closest_info(), searched, live)
        check_split_calls_and_counting(rtx, "capsule", tr, g, want, lambda info: 0 < info["lastPrimTests"] <= searched * live and info["lastNodeSteps"] > 0,
                                       unbounded_is_brute_force)


def _unbounded(g):
    u = g.copy()
    u["tMax"] = np.where(g["tMax"] > 0, np.float32(np.inf), g["tMax"])
    return u


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, g, want = cases("mixed")
    with rtx.MultiTracer([0] * 3) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        check_forms(rtx, mt, "capsule", g, want, "three contexts")
        kc.assert_same_records(rtx, ask(mt, "capsule", g[:1], 8, 0), want[8, 0][:1], "fewer segments than contexts")
        cc.assert_same_records(rtx, mt.closest_points(g), cc.oracle_closest(rtx, s, t, m, g), "three contexts, the defaults")


def test_device_entry_on_tensors_matches_the_checker():
    """(in a fresh process that imports torch first: tests/listed_torch_worker.py capsule)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "listed_torch_worker.py"), "capsule"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "capsule device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_a_point_segment_is_the_k_nearest_query(rtx, cases):
    """d = 0: every word but _reserved equals the K-nearest query of P0 wherever P0 is on or outside every sphere"""
    for name in ("two", "beside", "mixed"):
        s, t, m, g, _ = cases(name)
        q = g.copy()
        q["direction"] = 0
        outside = np.ones(len(q), bool)
        for sp in s:
            outside &= ~(np.linalg.norm(q["origin"].astype(np.float64) - sp["position"], axis=1) < float(sp["radius"]) * (1 + 1e-6))
        q = q[outside]
        with tracer_of(rtx, s, t, m) as tr:
            for f in ((8, 0), (3, 1)):
                got = kc.words(rtx, ask(tr, "capsule", q, *f)).copy()
                assert (got[..., kc.S_WORD] == 0).all()
                tr.set_option("closest_k", f[0])
                tr.set_option("closest_all", f[1])
                near = kc.words(rtx, tr.closest_points(q).reshape(len(q), f[0]))
                tr.set_option("closest_k", 1)
                tr.set_option("closest_all", 0)
                assert np.array_equal(got[..., :14], near[..., :14]), (name, f)
                assert np.array_equal(got[..., 14], near[..., 14])      # (and the count)


def test_refusals_and_the_mutual_exclusion(rtx, cases):
    s, t, m, g, want = cases("mixed")
    lib = rtx.load_library()
    with tracer_of(rtx, s, t, m) as tr, rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        for h in (tr, mt):
            h.set_option("closest_capsule", 1)
            h.set_option("closest_k", 3)
            h.set_option("closest_all", 1)
        stats, info = tr.stats(), tr.closest_info()
        for value in (2, -1):
            assert lib.rt_set_option(tr._ctx, b"closest_capsule", value) == -2 and b"closest_capsule" in lib.rt_last_error(tr._ctx), value
            assert lib.rt_multi_set_option(mt._m, b"closest_capsule", value) == -2 and b"closest_capsule" in lib.rt_multi_last_error(mt._m), value
        # a box while a capsule: refused, and both options keep their values
        assert lib.rt_set_option(tr._ctx, b"closest_box", 1) == -2 and b"closest_capsule" in lib.rt_last_error(tr._ctx)
        assert lib.rt_multi_set_option(mt._m, b"closest_box", 1) == -2
        assert all(np.array_equal(v, tr.stats()[k]) for k, v in stats.items()) and tr.closest_info() == info
        kc.assert_same_records(rtx, tr.closest_points(g).reshape(len(g), 3), want[3, 1], "after the refusals")
        kc.assert_same_records(rtx, mt.closest_points(g).reshape(len(g), 3), want[3, 1], "rt_multi after the refusals")
        # the other order: a capsule while a box
        tr.set_option("closest_capsule", 0)
        tr.set_option("closest_box", 1)
        assert lib.rt_set_option(tr._ctx, b"closest_capsule", 1) == -2 and b"closest_box" in lib.rt_last_error(tr._ctx)
        boxes = oc.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
        oc.assert_same_records(rtx, tr.closest_points(boxes).reshape(len(boxes), 3), oc.oracle_overlap(rtx, s, t, m, boxes, 3, 1), "still a box query")
        tr.set_option("closest_box", 0)
        tr.set_option("closest_capsule", 1)                     # (0 first, then 1: legal)
        kc.assert_same_records(rtx, tr.closest_points(g).reshape(len(g), 3), want[3, 1], "a capsule query again")


def test_the_option_at_0_after_1_gives_todays_bytes(rtx, cases):
    s, t, m, g, want = cases("mixed")
    q = g.copy()
    q["tMax"] = np.where(g["tMax"] > 0, np.float32(1.5), g["tMax"])
    boxes = oc.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
    with tracer_of(rtx, s, t, m) as tr:
        def others():
            out = [tr.closest_points(q).tobytes()]
            for f in nc.FORMS:
                tr.set_option("closest_k", f[0])
                tr.set_option("closest_all", f[1])
                out.append(tr.closest_points(q).tobytes())
                tr.set_option("closest_box", 1)
                out.append(tr.closest_points(boxes).tobytes())
                tr.set_option("closest_box", 0)
            tr.set_option("closest_k", 1)
            tr.set_option("closest_all", 0)
            out += [tr.trace_hits(q[:64], 4).tobytes(), tr.trace_rays(q[:64]).tobytes()]
            return out
        before = others()
        cc.assert_same_records(rtx, np.frombuffer(before[0], rtx.CLOSEST), cc.oracle_closest(rtx, s, t, m, q), "before the option")
        check_forms(rtx, tr, "capsule", g, want, "in between")
        assert others() == before
        # every other call ignores the option
        hits, rays = tr.trace_hits(q[:64], 4), tr.trace_rays(q[:64])
        tr.set_option("closest_capsule", 1)
        assert tr.trace_hits(q[:64], 4).tobytes() == hits.tobytes() and tr.trace_rays(q[:64]).tobytes() == rays.tobytes()


def test_a_call_moves_no_other_state(rtx, cases):
    _, _, _, g, want = cases("mixed")
    check_a_call_moves_no_other_state(rtx, "capsule", g, want)


def test_the_helpers_of_capsule_py(rtx, cases):
    s, t, m, g, _ = cases("mixed")
    ok = np.isfinite(g["origin"]).all(1) & np.isfinite(g["direction"]).all(1) & (np.abs(g["origin"]) < 1e30).all(1)
    g = g[ok]
    p0 = g["origin"]
    p1 = p0 + g["direction"]
    seg = kc.segments_of(rtx, p0, p1, 1.5)                      # (d = p1 - p0 again, as the helper forms it)
    with tracer_of(rtx, s, t, m) as tr:
        for k, count_all in ((4, 0), (2, 1)):
            got = rtx.capsule.overlap_capsule(tr, p0, p1, 1.5, k, count_all=bool(count_all))
            assert got.shape == (len(g), k)
            kc.assert_same_records(rtx, got, kc.oracle_capsule(rtx, s, t, m, seg, k, count_all), f"overlap_capsule {k} {count_all}")
        any_ = rtx.capsule.check_capsule(tr, p0, p1, 1.5)
        totals = kc.counts(kc.oracle_capsule(rtx, s, t, m, seg, 1, 1))[:, 0]
        assert any_.dtype == np.uint8 and np.array_equal(any_, (totals != 0).astype(np.uint8)) and 0 < any_.sum() < len(g)
        rec, par = rtx.capsule.closest_to_segment(tr, p0, p1)
        seg["tMax"] = np.inf
        want = kc.oracle_capsule(rtx, s, t, m, seg, 1, 0)[:, 0]
        kc.assert_same_records(rtx, rec.reshape(-1, 1), want.reshape(-1, 1), "closest_to_segment")
        assert par.dtype == np.float32 and np.array_equal(par.view(np.uint32), kc.params(want).view(np.uint32)) and ((par >= 0) & (par <= 1)).all()
        cc.assert_same_records(rtx, tr.closest_points(g), cc.oracle_closest(rtx, s, t, m, g), "the defaults are back")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        seg["tMax"] = 1.5
        kc.assert_same_records(rtx, rtx.capsule.overlap_capsule(mt, p0, p1, 1.5, 8), kc.oracle_capsule(rtx, s, t, m, seg, 8, 0), "on a MultiTracer")


def test_the_segments_bounds_prune(rtx):
    """8192 triangles; 512 vertical capsules (exact bound) and 512 along (1, 1, 1): node steps and primitive tests per query are a small
    fraction of the tree for both"""
    s, t, m = plane(rtx, 64, 64)
    rng = np.random.default_rng(3)
    n = 512
    cell = 8.0 / 64
    p0 = np.concatenate([rng.uniform(1, 7, (n, 2)), np.full((n, 1), cell)], 1)
    for name, d in (("vertical", (0, 0, 2 * cell)), ("diagonal", (2 * cell, 2 * cell, 2 * cell))):
        g = kc.segments_of(rtx, p0, d=np.repeat(np.float32([d]), n, 0), radius=1.5 * cell)
        with tracer_of(rtx, s, t, m, closest_count=1) as tr:
            kc.assert_same_records(rtx, ask(tr, "capsule", g, 8, 0), kc.oracle_capsule(rtx, s, t, m, g, 8, 0), f"plane of 8192, {name}")
            info, nodes = tr.closest_info(), tr.stats()["numBvhNodes"]
            print(f"{name}: node steps {info['lastNodeSteps'] / n:.2f} prim tests {info['lastPrimTests'] / n:.2f} per capsule of {nodes} nodes, {len(t)} triangles")
            # a capsule of reach 1.5 cells whose bounds span 2 cells meets at most 6 x 6 cells = 72 triangles: under 1/32 of the tree
            assert 0 < info["lastNodeSteps"] < n * nodes / 32 and 0 < info["lastPrimTests"] < n * len(t) / 32, info
