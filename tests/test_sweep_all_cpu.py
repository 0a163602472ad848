"""Sphere-cast-all without a GPU: the checker (tests/sweep_all_oracle.c) is pinned independently of the kernel, and the boundary is
checked.

The pin goes by another route than the checker's own loop: every primitive of a scene becomes a scene of its own, the sphere casts'
checker sw_cast (held to a float64 twin by tests/test_sweep_cpu.py) answers for each of them, and the hits, sorted here by (t, kind,
uploaded index), must be swa_cast's list word for word (words 0..12 and the feature code) with the count the number of hits.  K = 1 is
sw_cast on the whole scene, lists at K are prefixes of lists at larger K, hand cases on dyadic numbers fix side, ties, the strict tMax
and the rays that are not traced; and the batches the GPU tests trace are shown to fill, overflow and tie the list (conditions on the
batch, asserted here with the checker alone)."""
import os
import re

import numpy as np
import pytest

import sweep_all_check as sac
import sweep_check as sc
from test_camera_batch_cpu import built_library
from test_closest_cpu import scene
from test_gpu_closest import buffers_of
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata
from test_sweep_cpu import CUBE, T

NAMES = ("one", "two", "plane", "spheres", "mixed", "Knight")
INF = np.inf


@pytest.fixture(scope="module")
def batches(rtx):
    """name -> (spheres, triangles, meshinfo, rays, classes, the list at K = 8 with countAll), each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            rays, cls = sc.batch_of(rtx, s, t, m)
            deep = sac.oracle_cast_all(rtx, s, t, m, rays, 8, True)
            for a in (rays, cls, deep):
                a.setflags(write=False)
            cache[name] = (s, t, m, rays, cls, deep)
        return cache[name]
    return get


def one_primitive_lists(rtx, s, t, m, rays, K):
    """(uint32 (n, K, 14), counts (n,)): per ray the first K of the one-primitive scenes' sw_cast hits in ascending (t, kind, uploaded index)
    — words 0..12 and the feature code, chunk indices mapped back — and how many of the scenes were hit"""
    recs, kinds, prims = [], [], []
    for i in range(len(s)):
        hit, _ = sc.oracle_cast(rtx, s[i:i + 1], t[:0], m[:0], rays)
        hit = hit.copy()
        hit["primitive"][hit["kind"] != 0] = i
        recs.append(hit); kinds.append(1); prims.append(i)
    for c in range(len(m)):
        for j in range(int(m["numTriangles"][c])):
            ti = int(m["firstTriangleIndex"][c]) + j
            chunk = m[c:c + 1].copy()
            chunk["firstTriangleIndex"], chunk["numTriangles"] = ti, 1          # (the whole triangle buffer stays: the index is the uploaded one)
            hit, _ = sc.oracle_cast(rtx, s[:0], t, chunk, rays)
            hit = hit.copy()
            assert (hit["primitive"][hit["kind"] != 0] == ti).all()
            hit["chunk"][hit["kind"] != 0] = c
            recs.append(hit); kinds.append(2); prims.append(ti)
    n = len(rays)
    out = np.zeros((n, K, 14), np.uint32)
    counts = np.zeros(n, int)
    if not recs:
        return out, counts, np.zeros((n, K), bool)
    allr = np.stack(recs)                                                   # (primitives, n)
    w = allr.view(np.uint32).reshape(len(recs), n, 16)[:, :, :14]
    hit = allr["kind"] != 0
    kinds, prims = np.asarray(kinds), np.asarray(prims)
    filled = np.zeros((n, K), bool)
    for i in range(n):
        idx = np.flatnonzero(hit[:, i])
        counts[i] = len(idx)
        order = idx[np.lexsort((prims[idx], kinds[idx], allr["dst"][idx, i]))][:K]      # (float comparisons: -0.0 == 0.0)
        out[i, :len(order)] = w[order, i]
        filled[i, :len(order)] = True
    return out, counts, filled


def assert_pinned(rtx, s, t, m, rays, deep, what):
    want, counts, filled = one_primitive_lists(rtx, s, t, m, rays, 8)
    got = sac.words(deep)
    assert np.array_equal(deep[:, 0]["hitCount"], counts), what
    assert np.array_equal(deep["kind"] != 0, filled), what
    same = (got[:, :, :13] == want[:, :, :13]).all(2) & (got[:, :, 15] == want[:, :, 13])
    bad = np.argwhere(filled & ~same)
    assert len(bad) == 0, (what, len(bad), bad[:3], deep[tuple(bad[0])] if len(bad) else None)
    return int(filled.sum())


# ---- 1. the checker against the pinned checker, one primitive at a time -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "plane", "spheres", "mixed"])
def test_the_list_is_the_sorted_one_primitive_sphere_casts(rtx, batches, name):
    s, t, m, rays, _, deep = batches(name)
    assert len(rays) == 710
    records = assert_pinned(rtx, s, t, m, rays, deep, name)
    print(f"{name}: {records} records equal the one-primitive sphere casts")
    assert records > 100


def test_the_list_is_the_sorted_one_primitive_sphere_casts_on_the_knight(rtx, batches):
    """(every fifth ray: the product of 710 rays and 530 scenes is the slow part)"""
    s, t, m, rays, _, deep = batches("Knight")
    pick = np.arange(0, len(rays), 5)
    assert assert_pinned(rtx, s, t, m, rays[pick], deep[pick], "Knight") > 500


# ---- 2. K = 1, and prefixes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_k1_is_the_sphere_cast_and_lists_are_prefixes(rtx, batches, name):
    s, t, m, rays, _, deep = batches(name)
    first, occ = sc.oracle_cast(rtx, s, t, m, rays)
    lists = {(K, ca): sac.oracle_cast_all(rtx, s, t, m, rays, K, ca) for K in sac.KS for ca in (False, True)}
    k1 = lists[1, False][:, 0]
    w1, wf = sac.words(k1), first.view(np.uint32).reshape(-1, 16)
    assert np.array_equal(w1[:, :13], wf[:, :13]) and np.array_equal(w1[:, 15], wf[:, 13]), name
    assert np.array_equal(k1["hitCount"], occ.astype(np.int32))
    total = deep[:, 0]["hitCount"]
    for (K, ca), rec in lists.items():
        a, b = sac.words(rec).copy(), sac.words(deep[:, :K]).copy()
        assert np.array_equal(rec["hitCount"], np.broadcast_to((total if ca else np.minimum(total, K))[:, None], rec.shape)), (name, K, ca)
        a[:, :, 14] = b[:, :, 14] = 0                                       # (hitCount apart)
        assert np.array_equal(a, b), (name, K, ca)


# ---- 3. hand cases on dyadic numbers ----------------------------------------------------------------------------------------------------
def cast(rtx, sc_, o, d, r, t_max=INF, K=8, count_all=False):
    return sac.oracle_cast_all(rtx, *sc_, sc.rays_of(rtx, [o], [d], r, t_max), K, count_all)[0]


def keys(rec):
    """[(dst, kind, primitive, side, code), ...] of the filled records"""
    return [(float(r["dst"]), int(r["kind"]), int(r["primitive"]), int(r["side"]), int(r["_reserved"])) for r in rec if r["kind"] != 0]


def assert_empty(r, hit_count):
    assert np.isposinf(r["dst"]) and r["kind"] == 0 and r["primitive"] == -1 and r["chunk"] == -1 and r["mesh"] == -1 and r["side"] == 0
    assert (r["hitPoint"] == 0).all() and (r["normal"] == 0).all() and r["u"] == 0 and r["v"] == 0 and r["_reserved"] == 0 and r["hitCount"] == hit_count


def lowered(tri, dz):
    return tuple((x, y, z + dz) for x, y, z in tri)


def test_a_ball_dropped_through_two_stacked_faces(rtx):
    s = scene(rtx, [lowered(T, -2.0), T])                                   # the nearer face is uploaded second
    rec = cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0)
    assert keys(rec) == [(3.0, 2, 1, 1, 1), (5.0, 2, 0, 1, 1)] and all(r["hitCount"] == 2 for r in rec)
    assert tuple(rec[0]["hitPoint"]) == (1, -1, 0) and tuple(rec[1]["hitPoint"]) == (1, -1, -2) and tuple(rec[0]["normal"]) == (0, 0, 1)
    assert rec[0]["chunk"] == 0 and rec[0]["mesh"] == -1
    for r in rec[2:]:
        assert_empty(r, 2)
    # a direction of length 2 halves the travel
    assert [k[0] for k in keys(cast(rtx, s, (1, -1, 4), (0, 0, -2), 1.0))] == [1.5, 2.5]
    # from behind: the back faces, the centre below both at its contacts
    back = cast(rtx, s, (1, -1, -6), (0, 0, 1), 1.0)
    assert keys(back) == [(3.0, 2, 0, -1, 2), (5.0, 2, 1, -1, 2)] and tuple(back[0]["normal"]) == (0, 0, -1)
    assert back[0]["u"] == rec[1]["u"] and back[0]["v"] == rec[1]["v"] and tuple(back[0]["hitPoint"]) == (1, -1, -2)
    # K cuts the list; countAll counts what K cut
    assert keys(cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0, K=1)) == keys(rec)[:1]
    assert cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0, K=1)[0]["hitCount"] == 1
    assert cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0, K=1, count_all=True)[0]["hitCount"] == 2


def test_the_strict_tmax(rtx):
    s = scene(rtx, [lowered(T, -2.0), T])
    o, d = (1, -1, 4), (0, 0, -1)
    assert [k[0] for k in keys(cast(rtx, s, o, d, 1.0, 5.0))] == [3.0]
    assert [k[0] for k in keys(cast(rtx, s, o, d, 1.0, np.nextafter(np.float32(5), np.float32(6))))] == [3.0, 5.0]
    assert keys(cast(rtx, s, o, d, 1.0, 3.0)) == []
    assert cast(rtx, s, o, d, 1.0, 5.0, K=1, count_all=True)[0]["hitCount"] == 1      # countAll counts below tMax only


def test_a_ball_onto_a_cubes_edge_ties_the_two_faces_in_index_order(rtx):
    """the edge x = y = 0 belongs to triangle 4 (its AB) and triangle 8 (its AC): the same P and e, the same arithmetic, one t"""
    for chunks in (None, [(6, 6), (0, 6)]):                                 # (the uploaded index decides, not the chunk order)
        rec = cast(rtx, scene(rtx, CUBE, chunks=chunks), (-3, -3, 1), (1, 1, 0), 1.0, count_all=True)
        assert [(k[2], k[4]) for k in keys(rec)[:2]] == [(4, 3), (8, 4)]
        assert rec[0]["dst"].tobytes() == rec[1]["dst"].tobytes() and abs(rec[0]["dst"] - (3 - np.sqrt(0.5))) < 1e-6
        assert np.allclose(rec[0]["hitPoint"], (0, 0, 1), atol=1e-6) and rec[0]["hitPoint"].tobytes() == rec[1]["hitPoint"].tobytes()
        assert (rec[0]["u"], rec[0]["v"], rec[1]["u"], rec[1]["v"]) == (0.5, 0, 0, 0.5)
        # the ball goes on through the cube and touches every one of its twelve triangles; eight records hold the first eight
        assert keys(rec)[2][0] > keys(rec)[1][0] and len(keys(rec)) == 8 and (rec["hitCount"] == 12).all()
        # the centre is outside the cube, and this cube's faces look inwards (AB x AC of triangle 4 is +y on the face y = 0): behind both
        assert rec[0]["side"] == -1 and rec[1]["side"] == -1
        assert [k[2] for k in keys(cast(rtx, scene(rtx, CUBE, chunks=chunks), (-3, -3, 1), (1, 1, 0), 1.0, K=1))] == [4]


def test_a_sphere_and_a_triangle_at_one_t_the_sphere_first(rtx):
    s = scene(rtx, [T], [((9, 9, 9), 1.0), ((1, -1, -1), 1.0)])
    rec = cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0)
    assert keys(rec) == [(3.0, 1, 1, 1, 0), (3.0, 2, 0, 1, 1)]
    assert tuple(rec[0]["hitPoint"]) == (1, -1, 0) and tuple(rec[0]["normal"]) == (0, 0, 1) and rec[0]["chunk"] == -1 and rec[0]["u"] == 0
    assert keys(cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0, K=1)) == [(3.0, 1, 1, 1, 0)]


def test_the_six_rays_that_are_not_traced(rtx):
    s = scene(rtx, [T], [((1, -1, -4), 1.0)])
    for t_max, r in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (INF, 0.0), (INF, -1.0), (INF, np.nan), (INF, INF)):
        for count_all in (False, True):
            rec = cast(rtx, s, (1, -1, 4), (0, 0, -1), r, t_max, K=3, count_all=count_all)
            assert len(rec) == 3
            for x in rec:
                assert_empty(x, 0)
    assert len(keys(cast(rtx, s, (1, -1, 4), (0, 0, -1), 1.0))) == 2
    # a miss: K empty records with hitCount 0
    for x in cast(rtx, s, (1, -1, 4), (0, 0, 1), 1.0, K=2):
        assert_empty(x, 0)


# ---- 4. the batches exercise the list -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "Knight"])
def test_the_batches_fill_overflow_and_tie_the_list(rtx, batches, name):
    """conditions on the batch, not measurements of the kernel: sweep_check.batch_of's 710 rays meet them as they are"""
    s, t, m, rays, cls, deep = batches(name)
    traced = cls < 4
    total = deep[:, 0]["hitCount"]
    filled = deep["kind"] != 0
    bits = deep["dst"].view(np.uint32)
    tied = (filled[:, 1:] & (bits[:, 1:] == bits[:, :-1])).any(1)
    print(f"{name}: {int(traced.sum())} traced rays, {int((total[traced] >= 3).sum())} with three or more candidates, {int((total > 8).sum())} with "
          f"more than eight, {int(tied.sum())} with two records of bit-equal dst")
    assert (total[~traced] == 0).all()
    assert (total[traced] >= 3).sum() * 4 >= traced.sum()
    assert (total > 8).sum() >= 16
    assert tied.sum() >= 16


# ---- 5. boundary ----------------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_design_document_the_option_and_the_section():
    text = open(f"{ROOT}/include/rt.h").read()
    options = text[text.index("/* Tuning knobs"):text.index("int rt_set_option")]
    assert '"hits_sweep"' in options and "sphere-cast-all" in options
    section = text[text.index("/* ---- sphere-cast-all"):text.index("/* ---- feature buffers")]
    for word in ('"hits_sweep"', "rt_trace_hits", "rt_trace_hits_device", "rt_multi_trace_hits", "_reserved", "feature code", "CONTACT normal",
                 "g = r * (1 + 2^-6)", "(t, kind, primitive)", "-0.0f == 0.0f", "countAll", "side", "intersectMode plays no part",
                 '"hits_slice"', "first K records", '"sweep" = 1', "-2"):
        assert word in section, word
    assert text.index("/* ---- multi-hit ray queries") < text.index("/* ---- sphere-cast-all")
    design = open(f"{ROOT}/DESIGN.md").read()
    assert "### Sphere-cast-all" in design
    part = design[design.index("### Sphere-cast-all"):]
    for word in ("k_sweep_all", "sweep_node_step", "HitList", "K-th t", "VGPR", "isa_diff", "not measured"):
        assert word in part, word
    assert '"hits_sweep"' in open(f"{ROOT}/README.md").read() and "hits_sweep" in open(f"{ROOT}/INTEGRATION.md").read()


def test_the_surface_is_unchanged(rtx):
    assert len(rtx._cabi.SYMBOLS) == 115
    assert not any("sweep" in s or "sphere_cast" in s for s in rtx._cabi.SYMBOLS)
    for cls in (rtx.Tracer, rtx.MultiTracer):
        assert not any("sweep" in n or "sphere_cast" in n for n in dir(cls))
    assert callable(rtx.sweep.sphere_cast_all)
    cs = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs", "RtSweep.cs")).read()
    assert re.search(r"public\s+static\s+RtMultiHit\[\]\s+SphereCastAll\s*\(", cs) and '"hits_sweep"' in cs and "[DllImport" not in cs


def test_sphere_cast_all_refuses_bad_input_before_any_c_call(rtx):
    class Untouchable(rtx.Tracer):
        def __init__(self):
            pass

        def set_option(self, *a):
            raise AssertionError("a C call")
        trace_hits = trace_hits_device = set_option
    tr = Untouchable()
    rays = np.zeros(4, rtx.RAY)
    fn = rtx.sweep.sphere_cast_all
    for bad_rays, radius in ((np.zeros((4, 7), np.float32), 1.0), (np.zeros(4, np.float64), 1.0), (rays, np.ones(3)), (rays, np.ones((4, 1)))):
        with pytest.raises(ValueError):
            fn(tr, bad_rays, radius)
    for bad_k in (0, 9, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            fn(tr, rays, 1.0, bad_k)
    with pytest.raises(TypeError):
        fn(object(), rays, 1.0)

    class Recording(Untouchable):
        def __init__(self):
            self.log = []

        def set_option(self, name, value):
            self.log.append((name, value))

        def trace_hits(self, r, max_hits, both_sides, count_all):
            self.log.append(("trace_hits", max_hits, both_sides, count_all, sc.radii_of(r).tolist()))
            raise RuntimeError("the call failed")
    rec = Recording()
    with pytest.raises(RuntimeError):
        fn(rec, rays, [1.0, 2.0, 0.5, 4.0], 3, True)
    # the option is set for the one call and put back to 0 even when the call fails; "sweep" is not touched
    assert rec.log == [("hits_sweep", 1), ("trace_hits", 3, False, True, [1.0, 2.0, 0.5, 4.0]), ("hits_sweep", 0)]
    assert (rays["_reserved"] == 0).all()


def test_sweep_all_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_sweep_all" not in k[".name"]:
                continue
            names[k[".name"]] = k[".vgpr_count"]
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_sweep_all VGPRs:", names)
    assert len(names) == 2, sorted(names)           # f16 / f32 nodes
