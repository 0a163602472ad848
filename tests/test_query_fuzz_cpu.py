"""The query fuzz on the CPU (tests/query_fuzz.py): on the renderer fuzz's scenes every checker gives the same bits through the oracle's
search tree and through its literal loop, and the items have the power the GPU test (tests/test_gpu_query_fuzz.py) relies on — enough
hits, enough misses, closest hits with a second candidate at the bit-identical distance, and bounds one ulp either side of a hit.
The multi-hit and closest-point checkers, which have no tree, are pinned on these scenes to the ray-query checker (K = 1), to
themselves (the prefix property) and to a float64 twin, and their rays and points (qf.fuzz_points) have power of their own: rays with
many hits, points found and missed, ties at the winner's key, distances of exactly 0, radii one ulp either side of the distance."""
import os

import numpy as np
import pytest

import closest_check as cc
import hits_check as hc
import query_fuzz as qf
from query_check import assert_same_bits, oracle_candidates, oracle_hits
from ray_query_helpers import shim      # noqa: F401 (shim is a fixture)

SEEDS = range(24)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(rtx, shim):
    """seed -> (scene, items, options, call), built once"""
    return {seed: qf.fuzz_case(rtx, seed, shim) for seed in SEEDS}


@pytest.fixture(scope="module")
def counts(rtx, shim, cases):
    return {seed: qf.power_counts(rtx, cases[seed][0], cases[seed][1], shim) for seed in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_tree_against_loop(rtx, shim, cases, seed):
    scene, items, _, call = cases[seed]
    p, sph, tris, infos = scene
    mode = int(p["intersectMode"])
    tree = oracle_hits(rtx, shim, sph, tris, infos, mode, items, accel=True)
    loop = oracle_hits(rtx, shim, sph, tris, infos, mode, items)
    differ = np.where((tree.view(np.uint32).reshape(-1, 16) != loop.view(np.uint32).reshape(-1, 16)).any(1))[0]
    assert not len(differ), f"ray queries, seed {seed}: tree and loop differ, {qf.describe(items, differ[0])}: tree {tree[differ[0]]} loop {loop[differ[0]]}"
    for family, fmode in qf.FAMILIES:
        assert_same_bits(qf.checker(rtx, scene, items, call, family, fmode, accel=True),
                         qf.checker(rtx, scene, items, call, family, fmode, accel=False), f"{family} mode {fmode}, seed {seed}, {call}: tree vs loop")


@pytest.mark.parametrize("seed", SEEDS)
def test_every_seed_has_hits_and_misses(counts, seed):
    c = counts[seed]
    assert c["traced"] >= qf.N_ITEMS - 16, c
    assert 4 * c["hits"] >= c["traced"], f"seed {seed}: fewer than 25 % of the traced items hit: {c}"
    assert 10 * c["misses"] >= c["traced"], f"seed {seed}: fewer than 10 % of the traced items miss: {c}"


def test_ties_and_one_ulp_bounds_over_the_seeds(counts):
    ties, flips = sum(c["ties"] for c in counts.values()), sum(c["flips"] for c in counts.values())
    assert ties >= 200, f"{ties} closest hits with a second candidate at the same dst over {len(counts)} seeds"
    assert flips >= 50, f"{flips} hits that flip at tMax = dst +- 1 ulp over {len(counts)} seeds"


def test_the_recorded_counts_are_these(rtx, counts):
    """profiles/query_fuzz_inputs.txt holds what `python tests/query_fuzz.py` prints"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "query_fuzz_inputs.txt")):
        w = line.split()
        if len(w) == 10 and w[0].isdigit():
            rows[int(w[0])] = [int(x) for x in w[5:]]
    for seed, c in counts.items():
        assert rows[seed] == [c["traced"], c["hits"], c["misses"], c["ties"], c["flips"]], seed


def test_the_draw_is_a_function_of_the_seed_and_covers_every_value(rtx, shim, cases):
    scene, items, options, call = qf.fuzz_case(rtx, 5, shim)
    assert items.tobytes() == cases[5][1].tobytes() and options == cases[5][2] and call == cases[5][3]
    assert qf.fuzz_items(rtx, 5, shim=shim).tobytes() == items.tobytes()
    calls = [cases[s][3] for s in SEEDS]
    assert {c["samples"] for c in calls} == set(qf.SAMPLES) and {c["first_index"] for c in calls} == set(qf.FIRST_INDEX)
    assert {c["intersectMode"] for c in calls} == {0, 1}
    for name, values in (("lds_stack", {2, 3, 8, None}), ("radiance_slice", {1, 7, 100, None}), ("gather_slice", {1, 7, 100, None}),
                         ("visibility_slice", {1, 7, 100, None})):
        assert {cases[s][2].get(name) for s in SEEDS} == values, name
    # the degenerate handful: a NaN and an infinite origin, a zero and a NaN direction, tMax 0, -0, negative, NaN
    deg = items[-qf.N_DEGENERATE:]
    assert np.isnan(deg["origin"][0, 0]) and np.isinf(deg["origin"][1, 2]) and not deg["direction"][2].any() and np.isnan(deg["direction"][7, 1])
    assert deg["tMax"][3] == 0 and deg["tMax"][5] < 0 and np.isnan(deg["tMax"][6])
    # finite sources everywhere else, on a seed with a NaN triangle and on a shifted one
    for seed in (0, 4, 10, 21):
        body = cases[seed][1][:-qf.N_DEGENERATE]
        assert np.isfinite(body["origin"]).all() and not np.isnan(body["tMax"]).any(), seed
        assert np.abs(body["origin"] - qf.scene_shift(seed)).max() < 2e3, seed


# ---- rt_trace_hits and rt_closest_points: their inputs (qf.point_knobs, the items as rays, qf.fuzz_points) and their checkers ------------
SHARED = ("dst", "hitPoint", "normal", "kind", "primitive", "chunk", "mesh", "u", "v")      # of a ray-query hit and a multi-hit record
PERMUTED_SEED_WITH_A_THREE_WAY_TIE = 14


@pytest.fixture(scope="module")
def points(rtx, shim, cases):
    """seed -> (points, parts), built once"""
    out = {}
    for seed in SEEDS:
        parts = {}
        out[seed] = (qf.fuzz_points(rtx, seed, cases[seed][0], cases[seed][1], shim, parts), parts)
    return out


@pytest.fixture(scope="module")
def point_counts(rtx, shim, cases, points):
    return {seed: qf.point_power_counts(rtx, cases[seed][0], cases[seed][1], points[seed][0], shim) for seed in SEEDS}


def test_the_recorded_point_counts_are_these(rtx, point_counts):
    """profiles/query_fuzz_points.txt holds what `python tests/query_fuzz.py points` prints"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "query_fuzz_points.txt")):
        w = line.split()
        if len(w) == 1 + len(qf.POINT_COLUMNS) and w[0].isdigit():
            rows[int(w[0])] = [int(x) for x in w[1:]]
    assert sorted(rows) == list(SEEDS)
    for seed, c in point_counts.items():
        assert rows[seed] == [c[k] for k in qf.POINT_COLUMNS], seed


def test_the_point_draw_is_a_function_of_the_seed_and_covers_every_value(rtx, shim, cases, points):
    scene, items = cases[5][:2]
    assert qf.fuzz_points(rtx, 5, scene, items, shim).tobytes() == points[5][0].tobytes() and qf.point_knobs(5) == qf.point_knobs(5)
    knobs = [qf.point_knobs(s) for s in SEEDS]
    for name in ("hits_slice", "closest_slice"):
        assert {k[0].get(name) for k in knobs} == {1, 7, 100, None}, name
    assert {k[1]["K"] for k in knobs} == set(qf.HIT_K)
    assert {k[1]["both_sides"] for k in knobs} == {0, 1} and {k[1]["count_all"] for k in knobs} == {0, 1}
    radii = np.concatenate([points[s][0]["tMax"][slice(*points[s][1]["free"])] for s in SEEDS])
    assert np.isinf(radii).any() and (radii == np.float32(1.5)).any() and (radii == np.float32(3e20)).any() and (radii == np.float32(1e-30)).any()
    # the degenerate handful is the items': a NaN and an infinite coordinate, R of 0, -0, -1 and NaN
    pts = points[5][0]
    deg = pts[-qf.N_DEGENERATE:]
    assert np.isnan(deg["origin"][0, 0]) and np.isinf(deg["origin"][1, 2]) and deg["tMax"][3] == 0 and deg["tMax"][5] < 0 and np.isnan(deg["tMax"][6])
    assert len(pts) == qf.N_ITEMS and sum(qf.point_split(qf.N_ITEMS)[i] * (3 if i == 2 else 1) for i in range(5)) == qf.N_ITEMS
    # finite points everywhere else, within 2e3 of the scene, on a seed with a NaN triangle and on the shifted ones
    for seed in (0, 4, 10, 21):
        body = points[seed][0][:-qf.N_DEGENERATE]
        assert np.isfinite(body["origin"]).all() and not np.isnan(body["tMax"]).any() and not body["direction"].any(), seed
        assert np.abs(body["origin"] - qf.scene_shift(seed)).max() < 2e3, seed


@pytest.mark.parametrize("seed", SEEDS)
def test_every_seed_has_deep_rays_and_points_found_and_missed(point_counts, seed):
    c = point_counts[seed]
    assert c["two"] >= 64, f"seed {seed}: {c['two']} rays with two or more hits"
    assert c["untied"] >= 64, f"seed {seed}: {c['untied']} closest hits without a second candidate at their dst"
    assert c["searched"] >= qf.N_ITEMS - 40, c                                # (a flip below a dst of 0 is R = 0: not searched)
    assert 4 * c["found"] >= c["searched"], f"seed {seed}: fewer than 25 % of the searched points found: {c}"
    assert 10 * c["missed"] >= c["searched"], f"seed {seed}: fewer than 10 % of the searched points missed: {c}"


def test_point_ties_zero_distances_flips_and_long_lists_over_the_seeds(point_counts):
    total = {k: sum(c[k] for c in point_counts.values()) for k in qf.POINT_COLUMNS}
    assert total["deep"] >= 500, f"{total['deep']} rays with more than 8 hits over {len(point_counts)} seeds"
    assert total["tied"] >= 200 and total["zero"] >= 200 and total["flips"] >= 50, total


def test_a_permuted_chunk_list_has_a_three_way_tie(rtx, cases, points):
    seed = PERMUTED_SEED_WITH_A_THREE_WAY_TIE
    assert seed % 3 == 2
    _, sph, tris, infos = cases[seed][0]
    first = infos["firstTriangleIndex"].astype(np.int64)
    assert (np.diff(first) < 0).any(), "the chunk list is in upload order"
    at_best = cc.oracle_candidates(rtx, sph, tris, infos, points[seed][0])
    got = cc.oracle_closest(rtx, sph, tris, infos, points[seed][0])
    three = (at_best >= 3) & (got["kind"] == 2)
    assert three.sum() >= 8, int(three.sum())
    # ... and off the surface too: any point whose nearest surface is a "stack" triangle ties with its copies
    assert (three & (got["dst"] > 0)).sum() >= 4


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
def test_multihit_checker_k1_front_is_the_ray_query_checker(rtx, shim, cases, seed, intersect):
    """tests/test_hits_cpu.py's K = 1 pin on these scenes: word for word where the closest hit is untied (at a tie rt_trace_rays keeps
    the first chunk in the list, rt_trace_hits the lowest uploaded index: two definitions), hit or miss on every ray"""
    (_, sph, tris, infos), items = cases[seed][:2]
    want = oracle_hits(rtx, shim, sph, tris, infos, intersect, items)
    cand = oracle_candidates(rtx, shim, sph, tris, infos, intersect, items)
    got = hc.oracle_hits(rtx, sph, tris, infos, items, 1, hc.FRONT, False, intersect)[:, 0]
    assert ((got["hitCount"] == 1) == (want["dst"] < np.inf)).all() and (got["hitCount"] <= 1).all(), seed
    clear = cand < 2
    for f in SHARED:
        a, b = got[f][clear], want[f][clear]
        differ = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1))
        assert not len(differ), f"seed {seed}, intersect {intersect}, {f}: {qf.describe(items[clear], differ[0])}: {a[differ[0]]} against {b[differ[0]]}"


@pytest.mark.parametrize("seed", SEEDS)
def test_multihit_checker_prefix(rtx, cases, seed):
    """records 0 .. K-1 of the eight-record answer are the K-record answer (hitCount aside, which is capped at K unless all are counted)"""
    scene, items = cases[seed][:2]
    for both in (0, 1):
        for count_all in (0, 1):
            deep = qf.check_hits(rtx, scene, items, {"K": 8, "both_sides": both, "count_all": count_all})
            for K in (1, 2, 3):
                short = qf.check_hits(rtx, scene, items, {"K": K, "both_sides": both, "count_all": count_all})
                want = deep[:, :K].copy()
                if not count_all:
                    want["hitCount"] = np.minimum(want["hitCount"], K)
                hc.assert_same_records(rtx, short, want, f"seed {seed}, K {K} of 8, both sides {both}, countAll {count_all}")


@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 11 != 10] + [10, 21])
def test_closest_checker_against_the_float64_twin(rtx, cases, points, seed):
    """The checker sees the whole scene, the twin the triangles of its body only (nine finite coordinates within 1e4 of the shift): the
    checker never answers with one of the others, and its distance is the twin's within cc.dst_tolerance, evaluated on the two winners
    and the point — on the shifted seeds (10, 21) at coordinates of 2e5.  Every finite point, with R = inf."""
    _, sph, tris, infos = cases[seed][0]
    pts = points[seed][0].copy()
    pts = pts[np.isfinite(pts["origin"]).all(1)]
    pts["tMax"] = np.inf
    pos = np.stack([tris["posA"], tris["posB"], tris["posC"]], 1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        body = np.flatnonzero((np.isfinite(pos) & (np.abs(pos - qf.scene_shift(seed)) < 1e4)).all((1, 2)))
    addressed = np.zeros(len(tris), bool)
    for m in infos:
        addressed[int(m["firstTriangleIndex"]):int(m["firstTriangleIndex"]) + int(m["numTriangles"])] = True
    body = body[addressed[body]]
    A, B, C = pos[body, 0], pos[body, 1], pos[body, 2]
    c, r = np.asarray(sph["position"], np.float32).reshape(-1, 3), np.asarray(sph["radius"], np.float32)
    got = cc.oracle_closest(rtx, sph, tris, infos, pts)
    assert (got["kind"] != 0).all() and np.isin(got["primitive"][got["kind"] == 2], body).all(), seed
    worst = 0.0
    for g, p in zip(got, pts["origin"]):
        _, kind, prim, dst = cc.twin64(p, np.inf, c, r, A, B, C)
        mine = int(g["primitive"]) if g["kind"] == 1 else int(np.searchsorted(body, g["primitive"]))
        below = cc.dst_tolerance(p, int(g["kind"]), mine, c, r, A, B, C)[0]
        above = cc.dst_tolerance(p, int(kind[0]), int(prim[0]), c, r, A, B, C)[1]
        diff = float(g["dst"]) - dst
        worst = max(worst, abs(diff))
        assert -below <= diff <= above, f"seed {seed}, point {p.tolist()}: checker {g}, twin {dst!r} ({kind[0]}, {prim[0]}), allowed -{below:.3e} .. {above:.3e}"
    print(f"seed {seed}: {len(pts)} points, largest |dst - twin| {worst:.3e}")
