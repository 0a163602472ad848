"""Capsule overlap queries on the query fuzz's scenes (tests/query_fuzz.py: NaN and degenerate triangles, huge and tiny extents, empty
chunks, chunks out of order) with its builder options: segments drawn from its point batches — two fuzz points as the endpoints, a fuzz
point plus a tiny d, a fuzz point with d = 0 — in (K, all) drawn from the seed, every word of every record against
tests/capsule_oracle.c.  RTX_FUZZ_SEEDS / RTX_FUZZ_FIRST choose the seeds, as for test_gpu_fuzz.py."""
import os

import numpy as np
import pytest

import capsule_check as kc
import nearest_check as nc
import query_fuzz as qf
from ray_query_helpers import shim      # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

_FIRST = int(os.environ.get("RTX_FUZZ_FIRST", "0"))
_SEEDS = int(os.environ.get("RTX_FUZZ_SEEDS", "24"))


def fuzz_segments(rtx, seed, points):
    """the fuzz points as P0 with their radii; a third each: P1 = another fuzz point, d tiny against P0, d = 0"""
    rng = np.random.default_rng(1409 + seed)
    g = np.ascontiguousarray(points, rtx.RAY).copy()
    n = len(g)
    kind = rng.integers(0, 3, n)
    other = g["origin"][rng.permutation(n)]
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.where((kind == 0)[:, None], other - g["origin"], 0).astype(np.float32)
        tiny = (np.abs(g["origin"]) * np.float32(1e-6) + np.float32(1e-9)) * rng.choice(np.float32([-1, 0, 1]), (n, 3))
        d = np.where((kind == 1)[:, None], tiny.astype(np.float32), d)
    g["direction"] = d
    return g


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _SEEDS))
def test_capsules_on_a_random_scene(rtx, shim, seed):
    scene, items, options, _ = qf.fuzz_case(rtx, seed, shim)
    p, sph, tris, infos = scene
    more, _ = qf.point_knobs(seed)
    options = {**options, **more}
    segs = fuzz_segments(rtx, seed, qf.fuzz_points(rtx, seed, scene, items, shim))
    rng = np.random.default_rng(977 + seed)
    forms = [(int(rng.integers(1, 9)), 0), (int(rng.integers(1, 9)), 1)]
    ctx = f"fuzz seed {seed} ({len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres), options {options}"
    with rtx.Tracer(0) as t:                            # a context of its own: the options include the builder's
        qf.load_scene(t, scene, options)
        default = t.closest_points(segs)
        for k, count_all in forms:
            got = _ask(t, segs, k, count_all)           # (the options by hand: capsule.py would form d = p1 - p0 again)
            kc.assert_same_records(rtx, got, kc.oracle_capsule(rtx, sph, tris, infos, segs, k, count_all), f"K {k} all {count_all}, {ctx}")
        nc.assert_same_records(rtx, t.closest_points(segs), default, "the defaults again, " + ctx)


def _ask(t, segs, k, count_all):
    t.set_option("closest_capsule", 1)
    t.set_option("closest_k", k)
    t.set_option("closest_all", count_all)
    try:
        return t.closest_points(segs).reshape(len(segs), k)
    finally:
        t.set_option("closest_capsule", 0)
        t.set_option("closest_k", 1)
        t.set_option("closest_all", 0)
