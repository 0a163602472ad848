"""The image chain (rt_render_aov, rt_denoise, rt_denoise_variance, rt_temporal, rt_denoise_temporal and their rt_multi forms) on the
renderer fuzz's scenes extended by what is hostile to the filters (tests/filter_fuzz.py): vertex normals that normalise to NaN, 0 or an
infinity, depths of 1e15 .. 4e18 and of half a millimetre, albedos that are 0, negative, 1e30, infinite or NaN, invisible lights in
front of and coincident with ordinary quads, a sliver of coverage, all three sample-lane layouts, a permuted chunk list; sigmas whose
square overflows or underflows, every iteration count, tolerances of 1e-30 and 1e30, history caps from 1 to 4096; a pose sequence that
stands still, steps so that a column reprojects to weights below 0.01, zooms and turns away.  Every plane of every call equals its CPU
checker bit for bit (NaN equal to NaN; tests/test_filter_fuzz_cpu.py shows on the checkers alone that more than half of every output is
finite and that every hostile class occurs), the filter calls move nothing else, and on every third seed an rt_multi of three contexts
gives the single context's bits.  RTX_FUZZ_SEEDS / RTX_FUZZ_FIRST choose the seeds, as for test_gpu_fuzz.py.
Measured on an MI355X: 2.73 s for the 24 default seeds (0.73 s the first, which loads the code object, about 0.09 s a plain one),
13.83 s for 200 (profiles/filter_fuzz_soak.txt).  The test starts no process and sets no time limit of its own."""
import os

import pytest

import filter_fuzz as ff
from aov_check import assert_same_bits
from test_gpu_denoise import assert_same_state, state_of

pytestmark = pytest.mark.gpu

_FIRST = int(os.environ.get("RTX_FUZZ_FIRST", "0"))
_SEEDS = int(os.environ.get("RTX_FUZZ_SEEDS", "24"))       # RTX_FUZZ_SEEDS=200 for a soak run


@pytest.mark.parametrize("seed", range(_FIRST, _FIRST + _SEEDS))
def test_image_chain_on_a_hostile_scene(rtx, seed):
    case = ff.fuzz_case(rtx, seed)
    p, sph, tris, infos = case["scene"]
    ctx = (f"fuzz seed {seed} ({int(p['width'])} x {int(p['height'])}, {int(p['numRaysPerPixel'])} samples, {len(tris)} triangles in {len(infos)} chunks, "
           f"{len(sph)} spheres), options {case['knobs']['options']}")
    kept = {}

    def state(t, name):
        """the state the header says a filter call leaves: snapshot at "before ...", compared at "after ..." """
        if name.startswith("before"):
            kept["state"] = state_of(t)
        else:
            assert_same_state(state_of(t), kept["state"], f"{name}, {ctx}")

    single = []
    t = rtx.Tracer(0)                                    # a context of its own: the options include the builder's
    try:
        ff.load_scene(t, case)
        for name, got, want, _ in ff.stages(rtx, t, case, state):
            assert_same_bits(got, want(), f"{name}, {ctx}")
            single.append((name, got))
    finally:
        t.close()
    # ---- through an rt_multi of three contexts on the device: the band split, the gather with its halo rows
    if seed % 3 == 0:
        with rtx.MultiTracer([0] * 3) as m:
            ff.load_scene(m, case)
            for (name, got, _, _), (name1, want) in zip(ff.stages(rtx, m, case), single):
                assert name == name1
                assert_same_bits(got, want, f"rt_multi {name}, {ctx}")
