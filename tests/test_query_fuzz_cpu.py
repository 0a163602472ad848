"""The query fuzz on the CPU (tests/query_fuzz.py): on the renderer fuzz's scenes every checker gives the same bits through the oracle's
search tree and through its literal loop, and the items have the power the GPU test (tests/test_gpu_query_fuzz.py) relies on — enough
hits, enough misses, closest hits with a second candidate at the bit-identical distance, and bounds one ulp either side of a hit."""
import os

import numpy as np
import pytest

import query_fuzz as qf
from query_check import assert_same_bits, oracle_hits
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
