"""K-nearest point queries on the query fuzz's scenes (tests/query_fuzz.py: NaN and degenerate triangles, huge and tiny extents,
empty chunks, chunks out of order) with its builder options and point batches: (K, all) drawn from the seed, every word of every
record against tests/nearest_oracle.c, and record 0 against the default rt_closest_points call on the same context.
RTX_FUZZ_SEEDS / RTX_FUZZ_FIRST choose the seeds, as for test_gpu_fuzz.py."""
import os

import numpy as np
import pytest

import nearest_check as nc
import query_fuzz as qf
from ray_query_helpers import shim      # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

_FIRST = int(os.environ.get("RTX_FUZZ_FIRST", "0"))
_SEEDS = int(os.environ.get("RTX_FUZZ_SEEDS", "24"))


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _SEEDS))
def test_k_nearest_on_a_random_scene(rtx, shim, seed):
    scene, items, options, _ = qf.fuzz_case(rtx, seed, shim)
    p, sph, tris, infos = scene
    more, _ = qf.point_knobs(seed)
    options = {**options, **more}
    points = qf.fuzz_points(rtx, seed, scene, items, shim)
    rng = np.random.default_rng(977 + seed)
    forms = [(int(rng.integers(2, 9)), 0), (int(rng.integers(1, 9)), 1)]
    ctx = f"fuzz seed {seed} ({len(tris)} triangles in {len(infos)} chunks, {len(sph)} spheres), options {options}"
    with rtx.Tracer(0) as t:                            # a context of its own: the options include the builder's
        qf.load_scene(t, scene, options)
        default = t.closest_points(points)
        assert default.shape == (len(points),) and (default["_reserved"] == 0).all()
        for k, count_all in forms:
            got = rtx.nearest.nearest_k(t, points, k, count_all=bool(count_all))
            what = f"K {k} all {count_all}, {ctx}"
            nc.assert_same_records(rtx, got, nc.oracle_nearest(rtx, sph, tris, infos, points, k, count_all), what)
            nc.assert_first_is_the_default(rtx, got, default, what)
        nc.assert_same_records(rtx, t.closest_points(points), default, "the defaults again, " + ctx)
