"""Box overlap queries on the GPU (rt_closest_points and its device and rt_multi forms with the option "closest_box"): every word of
every record bit for bit against the brute-force checker (tests/overlap_oracle.c, pinned by tests/test_overlap_cpu.py), over
test_gpu_closest's scenes with overlap_check.batch_of's boxes (whole triangles inside, pierced by the interior, separated by an edge
axis alone, faces on vertices bit for bit, point boxes, the whole scene, nothing, inputs that are not searched), in the forms
(K, all) = (2, 0), (8, 0), (3, 1), (1, 1): both node forms, both builders, every leaf size, scenes far from the origin, a traversal
stack that spills, a refitted local-mesh scene, invisible slicing, rt_multi, the device entry; refusals; the defaults; the state a call
leaves alone; that the box and the K-th key prune; the helpers of overlap.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_check as cc
import nearest_check as nc
import overlap_check as oc
from listed_gpu import ask, check_a_call_moves_no_other_state, check_forms, check_split_calls_and_counting, make_cases
from ray_query_helpers import scene_of
from test_gpu_closest import NAMES, batch_of, buffers_of, plane, tracer_of
from test_gpu_ray_query import local_tracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(rtx):
    """name -> (spheres, triangles, meshinfo, boxes, {(K, all): the checker's answer}), each computed once"""
    return make_cases(rtx, "overlap", buffers_of)


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("compact_nodes", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_scenes_node_forms_and_builders(rtx, cases, name, compact_nodes, device_bvh):
    s, t, m, p, want = cases(name)
    with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, device_bvh=device_bvh, max_leaf=1 if name == "plane" else 2) as tr:
        check_forms(rtx, tr, "overlap", p, want, f"{name} compact_nodes {compact_nodes} device_bvh {device_bvh}")
        if name == "plane":
            assert tr.stats()["numBvhNodes"] > 5                # (several levels)


@pytest.mark.parametrize("max_leaf", [1, 2, 3, 4])
def test_leaf_sizes(rtx, cases, max_leaf):
    s, t, m, p, want = cases("one")
    with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
        check_forms(rtx, tr, "overlap", p, want, f"one max_leaf {max_leaf}", [(8, 0), (1, 1)])
    for name in ("plane", "Knight"):
        s, t, m, p, want = cases(name)
        with tracer_of(rtx, s, t, m, max_leaf=max_leaf) as tr:
            check_forms(rtx, tr, "overlap", p, want, f"{name} max_leaf {max_leaf}", [(8, 0)])


@pytest.mark.parametrize("name", ["two", "mixed", "Knight"])
def test_scene_and_boxes_far_from_the_origin(rtx, cases, name):
    """everything translated by (1e4, -1e4, 1e4): the boxes stay small while coordinates are large"""
    s, t, m, p, _ = cases(name)
    off = np.array([1e4, -1e4, 1e4], np.float32)
    s2, t2, m2, p2 = s.copy(), t.copy(), m.copy(), p.copy()
    s2["position"] += off
    for k in ("posA", "posB", "posC"):
        t2[k] += off
    m2["boundsMin"] += off
    m2["boundsMax"] += off
    p2["origin"] += off
    want = {f: oc.oracle_overlap(rtx, s2, t2, m2, p2, *f) for f in ((8, 0), (3, 1))}
    assert (oc.counts(want[3, 1])[:, 0] > 0).sum() > 100
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s2, t2, m2, compact_nodes=compact_nodes) as tr:
            check_forms(rtx, tr, "overlap", p2, want, f"{name} translated, compact_nodes {compact_nodes}", list(want))


@pytest.mark.parametrize("compact_nodes", [0, 1])
def test_small_lds_stack_spills_to_the_overflow_area(rtx, cases, compact_nodes):
    s, t, m, p, want = cases("Knight")
    with tracer_of(rtx, s, t, m, stream_stack=4, lds_stack=3, compact_nodes=compact_nodes, max_leaf=1) as tr:
        check_forms(rtx, tr, "overlap", p, want, f"lds_stack 3, compact_nodes {compact_nodes}", [(8, 0), (3, 1)])
        assert tr.stats()["bvhMaxStack"] > 3                    # (the overflow area was in use)


@pytest.mark.parametrize("device_bvh", [0, 1])
def test_local_meshes_after_a_refit(rtx, device_bvh):
    tr, params, s, world, infos, chunk_mesh = local_tracer(rtx, scene_of(rtx, "mesh_test_scene"), device_bvh=device_bvh)
    with tr:
        p = oc.batch_of(rtx, s, world, infos, batch_of(rtx, s, world, infos, seed=5))
        for f in ((8, 0), (3, 1)):
            got = ask(tr, "overlap", p, *f)
            oc.assert_same_records(rtx, got, oc.oracle_overlap(rtx, s, world, infos, p, *f, chunk_mesh=chunk_mesh), f"local meshes, device_bvh {device_bvh}, {f}")
        tri = got[got["kind"] == 2]
        assert len(tri) > 100 and (tri["mesh"] >= 0).all() and len(np.unique(tri["mesh"])) > 1


def test_slices_split_calls_and_counting_are_invisible(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with tracer_of(rtx, s, t, m) as tr:
        tr.set_option("closest_slice", 7)
        check_forms(rtx, tr, "overlap", p[:150], {f: w[:150] for f, w in want.items()}, "closest_slice 7")
        tr.set_option("closest_slice", 333)
        check_forms(rtx, tr, "overlap", p, want, "closest_slice 333", [(8, 0)])
        touching = int(oc.counts(want[3, 1])[:, 0].sum())
        check_split_calls_and_counting(rtx, "overlap", tr, p, want, lambda info: info["lastPrimTests"] >= touching and info["lastNodeSteps"] > 0)


def test_multi_tracer_gives_the_single_context_bits(rtx, cases):
    s, t, m, p, want = cases("mixed")
    with rtx.MultiTracer([0] * 3) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        check_forms(rtx, mt, "overlap", p, want, "three contexts")
        oc.assert_same_records(rtx, ask(mt, "overlap", p[:1], 8, 0), want[8, 0][:1], "fewer boxes than contexts")
        cc.assert_same_records(rtx, mt.closest_points(p), cc.oracle_closest(rtx, s, t, m, p), "three contexts, the defaults")


def test_device_entry_on_tensors_matches_the_checker():
    """(in a fresh process that imports torch first: tests/listed_torch_worker.py overlap)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "listed_torch_worker.py"), "overlap"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "overlap device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals_leave_the_option_and_every_state_alone(rtx, cases):
    s, t, m, p, want = cases("mixed")
    lib = rtx.load_library()
    with tracer_of(rtx, s, t, m) as tr, rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        for h in (tr, mt):
            h.set_option("closest_box", 1)
            h.set_option("closest_k", 3)
            h.set_option("closest_all", 1)
        stats, info = tr.stats(), tr.closest_info()
        for value in (2, -1):
            assert lib.rt_set_option(tr._ctx, b"closest_box", value) == -2 and b"closest_box" in lib.rt_last_error(tr._ctx), value
            assert lib.rt_multi_set_option(mt._m, b"closest_box", value) == -2 and b"closest_box" in lib.rt_multi_last_error(mt._m), value
        assert all(np.array_equal(v, tr.stats()[k]) for k, v in stats.items()) and tr.closest_info() == info
        # the option kept its value: the next call is still a box query at (3, 1)
        oc.assert_same_records(rtx, tr.closest_points(p).reshape(len(p), 3), want[3, 1], "after the refusals")
        oc.assert_same_records(rtx, mt.closest_points(p).reshape(len(p), 3), want[3, 1], "rt_multi after the refusals")


def test_the_option_at_0_after_1_gives_todays_bytes(rtx, cases):
    s, t, m, p, want = cases("mixed")
    q = p.copy()
    q["tMax"] = np.where(p["tMax"] > 0, np.float32(1.5), p["tMax"])        # (as points: a radius that takes in several candidates)
    default = cc.oracle_closest(rtx, s, t, m, q)
    nearest = {f: nc.oracle_nearest(rtx, s, t, m, q, *f) for f in nc.FORMS}
    with tracer_of(rtx, s, t, m) as tr:
        got = tr.closest_points(q)
        assert got.shape == (len(q),) and (got["_reserved"] == 0).all()
        cc.assert_same_records(rtx, got, default, "before the option")
        check_forms(rtx, tr, "overlap", p, want, "in between")
        tr.set_option("closest_box", 1)
        tr.set_option("closest_box", 0)
        again = tr.closest_points(q)
        assert again.shape == (len(q),) and again.tobytes() == got.tobytes()
        for f in nc.FORMS:                                      # K-nearest, with the box option back at 0
            tr.set_option("closest_k", f[0])
            tr.set_option("closest_all", f[1])
            nc.assert_same_records(rtx, tr.closest_points(q).reshape(len(q), f[0]), nearest[f], f"K-nearest {f} after box queries")
        tr.set_option("closest_k", 1)
        tr.set_option("closest_all", 0)
        # every other call ignores the option: the same hits and rays with it set
        hits, rays = tr.trace_hits(q[:64], 4), tr.trace_rays(q[:64])
        tr.set_option("closest_box", 1)
        assert tr.trace_hits(q[:64], 4).tobytes() == hits.tobytes() and tr.trace_rays(q[:64]).tobytes() == rays.tobytes()


def test_a_call_moves_no_other_state(rtx, cases):
    _, _, _, p, want = cases("mixed")
    check_a_call_moves_no_other_state(rtx, "overlap", p, want)


def test_the_box_and_the_kth_key_prune(rtx):
    """8192 triangles, 1024 cell-sized boxes on them.  (1, 1): only the box culls, and the node steps and primitive tests per box are a
    small fraction of the tree; (8, 0): the K-th key culls as well, so it does no more."""
    s, t, m = plane(rtx, 64, 64)
    rng = np.random.default_rng(3)
    n = 1024
    cell = 8.0 / 64
    boxes = oc.boxes_of(rtx, np.concatenate([rng.uniform(0, 8, (n, 2)), rng.uniform(-cell / 4, cell / 4, (n, 1))], 1), cell / 2)
    for compact_nodes in (0, 1):
        with tracer_of(rtx, s, t, m, compact_nodes=compact_nodes, closest_count=1) as tr:
            oc.assert_same_records(rtx, ask(tr, "overlap", boxes, 1, 1), oc.oracle_overlap(rtx, s, t, m, boxes, 1, 1), "plane of 8192, (1, 1)")
            by_box = tr.closest_info()
            nodes = tr.stats()["numBvhNodes"]
            oc.assert_same_records(rtx, ask(tr, "overlap", boxes, 8, 0), oc.oracle_overlap(rtx, s, t, m, boxes, 8, 0), "plane of 8192, (8, 0)")
            by_key = tr.closest_info()
            print(f"compact_nodes {compact_nodes}: {nodes} nodes, {len(t)} triangles; per box at (1, 1) node steps {by_box['lastNodeSteps'] / n:.2f} "
                  f"prim tests {by_box['lastPrimTests'] / n:.2f}; at (8, 0) node steps {by_key['lastNodeSteps'] / n:.2f} prim tests {by_key['lastPrimTests'] / n:.2f}")
            # "a small fraction of the tree": under 1/32 of its nodes and of its triangles (a cell-sized box meets at most 3 x 3 cells = 18
            # triangles and the nodes above them; the tree has 8192 triangles)
            assert 0 < by_box["lastNodeSteps"] < n * nodes / 32 and 0 < by_box["lastPrimTests"] < n * len(t) / 32, by_box
            assert by_key["lastNodeSteps"] <= by_box["lastNodeSteps"] and by_key["lastPrimTests"] <= by_box["lastPrimTests"], (by_key, by_box)


def test_the_helpers_of_overlap_py(rtx, cases):
    s, t, m, p, want = cases("mixed")
    gate = p.copy()
    gate["tMax"] = 1.0                                          # (the helpers' gate is always open)
    with tracer_of(rtx, s, t, m) as tr:
        for k, count_all in oc.FORMS:
            got = rtx.overlap.overlap_box(tr, p["origin"], p["direction"], k, count_all=bool(count_all))
            assert got.shape == (len(p), k)
            oc.assert_same_records(rtx, got, oc.oracle_overlap(rtx, s, t, m, gate, k, count_all), f"overlap_box {k} {count_all}")
        any_ = rtx.overlap.check_box(tr, p["origin"], p["direction"])
        assert any_.dtype == np.uint8 and any_.shape == (len(p),)
        totals = oc.counts(oc.oracle_overlap(rtx, s, t, m, gate, 1, 1))[:, 0]
        assert np.array_equal(any_, (totals != 0).astype(np.uint8)) and 0 < any_.sum() < len(p)
        # voxel_counts: an 8 x 8 x 8 grid over the scene's bounds against the checker on the same cell boxes
        lo, hi = (x.astype(np.float32) for x in oc.scene_bounds(s, t, m))
        v = rtx.overlap.voxel_counts(tr, lo, hi, (8, 8, 8))
        assert v.shape == (8, 8, 8) and v.dtype == np.int32
        cell = (hi - lo) / np.float32([8, 8, 8])
        ijk = np.stack(np.unravel_index(np.arange(512), (8, 8, 8)), 1).astype(np.float32)
        cells = oc.boxes_of(rtx, lo + (ijk + np.float32(0.5)) * cell, cell * np.float32(0.5))
        assert np.array_equal(v.reshape(-1), oc.counts(oc.oracle_overlap(rtx, s, t, m, cells, 1, 1))[:, 0]) and 0 < (v > 0).sum() < 512
        cc.assert_same_records(rtx, tr.closest_points(p), cc.oracle_closest(rtx, s, t, m, p), "the defaults are back")
    with rtx.MultiTracer([0] * 2) as mt:
        mt.upload(spheres=s, triangles=t, meshinfo=m)
        oc.assert_same_records(rtx, rtx.overlap.overlap_box(mt, p["origin"], p["direction"], 8), oc.oracle_overlap(rtx, s, t, m, gate, 8, 0), "overlap_box on a MultiTracer")
        assert np.array_equal(rtx.overlap.voxel_counts(mt, lo, hi, (8, 8, 8)), v)
