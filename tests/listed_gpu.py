"""The frame the GPU tests of the listed point queries share — test_gpu_nearest.py, test_gpu_overlap.py and test_gpu_capsule.py: a family
is the option that selects it, its checker module and its oracle; the cached cases of a module, the one call with the options set and
put back, the comparison over the forms, and the bodies of the tests that are the same for the three.  Each module keeps its scenes,
forms, thresholds and every test function; tests/listed_torch_worker.py uses the families too.  Neither a test module nor a conftest."""
import collections

import numpy as np

import capsule_check as kc
import nearest_check as nc
import overlap_check as oc
from ray_query_helpers import scene_of
from test_gpu_closest import STATS_MAY_MOVE, batch_of

Family = collections.namedtuple("Family", "option check oracle")      # option: None for K-nearest, which "closest_k" alone selects
FAMILIES = {"nearest": Family(None, nc, nc.oracle_nearest), "overlap": Family("closest_box", oc, oc.oracle_overlap),
            "capsule": Family("closest_capsule", kc, kc.oracle_capsule)}


def make_cases(rtx, family, scene_fn):
    """name -> (spheres, triangles, meshinfo, inputs, {(K, all): the checker's answer}), each computed once; scene_fn(rtx, name) gives the
    first three"""
    fam = FAMILIES[family]
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = scene_fn(rtx, name)
            p = fam.check.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
            want = {f: fam.oracle(rtx, s, t, m, p, *f) for f in fam.check.FORMS}
            for a in (p, *want.values()):
                a.setflags(write=False)
            cache[name] = (s, t, m, p, want)
        return cache[name]
    return get


def ask(tr, family, inputs, k, count_all):
    """closest_points with the family's options set for the one call; (n, K) whatever K"""
    option = FAMILIES[family].option
    if option:
        tr.set_option(option, 1)
    tr.set_option("closest_k", k)
    tr.set_option("closest_all", count_all)
    try:
        return tr.closest_points(inputs).reshape(len(inputs), k)
    finally:
        if option:
            tr.set_option(option, 0)
        tr.set_option("closest_k", 1)
        tr.set_option("closest_all", 0)


def check_forms(rtx, tr, family, inputs, want, what, forms=None):
    fam = FAMILIES[family]
    for f in fam.check.FORMS if forms is None else forms:
        fam.check.assert_same_records(rtx, ask(tr, family, inputs, *f), want[f], f"{what}, (K, all) = {f}")


def check_a_call_moves_no_other_state(rtx, family, inputs, want, then=None):
    """a context that holds an image, feature planes, a filtered image, a temporal history and the other queries' counters: the family's
    calls, one per form, leave every one of them alone (the far inputs may widen the padding: STATS_MAY_MOVE).  then(tb): what a module
    checks beside, on the same context"""
    params, s, t, m = scene_of(rtx, "mesh_test_scene").build_buffers()
    with rtx.Tracer(0) as tb:
        tb.set_params(params)
        tb.upload(spheres=s, triangles=t, meshinfo=m)
        tb.render(0, 2)
        tb.render_aov(0, 2)
        tb.denoise(iterations=2)
        tb.temporal()
        tb.visibility(inputs[:64], 4)
        tb.trace_hits(inputs[:64], 4)

        def state():
            return {"accum": tb.read_accum(), "last": tb.read_last_frame(), "albedo": tb.read_aov(0), "normal_depth": tb.read_aov(1),
                    "denoised": tb.read_denoised(), "temporal": tb.read_temporal(), "history": tb.read_temporal_history(),
                    "aov_info": tb.aov_info(), "denoise_info": tb.denoise_info(), "temporal_info": tb.temporal_info(),
                    "radiance_info": tb.radiance_info(), "gather_info": tb.gather_info(), "visibility_info": tb.visibility_info(),
                    "hits_info": tb.hits_info(), "stats": tb.stats()}
        before = state()
        assert tb.closest_info()["calls"] == 0
        check_forms(rtx, tb, family, inputs, want, "beside an image")
        assert tb.closest_info()["calls"] == len(FAMILIES[family].check.FORMS)
        after = state()
        for k in ("accum", "last", "albedo", "normal_depth", "denoised", "temporal", "history"):
            assert before[k].tobytes() == after[k].tobytes(), k
        for k in ("aov_info", "denoise_info", "temporal_info", "radiance_info", "gather_info", "visibility_info", "hits_info"):
            assert before[k] == after[k], k
        for k, v in before["stats"].items():
            if k not in STATS_MAY_MOVE:
                assert np.array_equal(v, after["stats"][k]), k
        if then:
            then(tb)


def check_split_calls_and_counting(rtx, family, tr, inputs, want, counted, while_counting=None):
    """after a module's own slice settings: a batch cut in two calls gives the bits of one; without "closest_count" nothing is counted;
    with it every form keeps its bits and counted(info) holds — the family's own bound — and without it again nothing is counted"""
    fam = FAMILIES[family]
    tr.set_option("closest_slice", 1 << 22)
    for cut in (1, 333):
        for f in ((8, 0), (3, 1)):
            fam.check.assert_same_records(rtx, np.concatenate([ask(tr, family, inputs[:cut], *f), ask(tr, family, inputs[cut:], *f)]), want[f], f"cut at {cut}, {f}")
    assert tr.closest_info()["lastPrimTests"] == 0 and tr.closest_info()["lastNodeSteps"] == 0
    tr.set_option("closest_count", 1)
    for f in fam.check.FORMS:
        fam.check.assert_same_records(rtx, ask(tr, family, inputs, *f), want[f], f"the counting kernel, {f}")
        info = tr.closest_info()
        assert counted(info), info
    if while_counting:
        while_counting()
    tr.set_option("closest_count", 0)
    check_forms(rtx, tr, family, inputs, want, "after the counting kernel", [(2, 0)])
    assert tr.closest_info()["lastPrimTests"] == 0
