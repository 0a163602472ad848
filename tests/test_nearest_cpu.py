"""K-nearest point queries without a GPU: the header and DESIGN.md document the options and the section, nearest.py refuses bad input
before any C call, the symbol count is unchanged, the four k_nearest instantiations are built without scratch, and the checker
(tests/nearest_oracle.c) is pinned independently of the kernel — against the closest-point checker, the prefix property, hand cases
on dyadic numbers, a float64 twin, a closed-form count, and five one-line mutants, each of which some hand case tells from it.

The float64 twin.  closest_check.dst_tolerance gives, for ONE primitive, how far the checker's float32 distance can lie from the exact
one: (below, above).  With tol = the largest of both over ALL primitives of a case, every float32 distance is within tol of its exact
value, so the j-th smallest of the one list is within tol of the j-th smallest of the other (order statistics move by at most the
largest move): distances are compared, not identities, because near-ties may swap.  The count of a bounded search lies between the
twin's counts of dst < R - tol and dst < R + tol."""
import os

import numpy as np
import pytest

import cabi_record
import closest_check as cc
import nearest_check as nc
from test_camera_batch_cpu import built_library
from test_closest_cpu import T0, _random_case, scene
from test_gpu_closest import NAMES, batch_of, buffers_of, plane
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata
from test_sweep_cpu import CUBE


def near(rtx, sc, p, R=np.inf, k=8, count_all=0, variant=nc.DEFINITION):
    """the K records of one point"""
    return nc.oracle_nearest(rtx, *sc, cc.points_of(rtx, [p], R), k, count_all, variant=variant)[0]


def counts(r):
    return r["_reserved"][..., 0]


# ---- documentation and surface ----------------------------------------------------------------------------------------------------------
def test_the_header_documents_the_options_and_the_section():
    text = open(f"{ROOT}/include/rt.h").read()
    options = text[text.index("int rt_set_option") - 14000:text.index("int rt_set_option")]
    assert '"closest_k"' in options and '"closest_all"' in options and "K-nearest queries" in options
    section = text[text.index("/* ---- K-nearest queries"):text.index("/* ---- multi-hit ray queries")]
    assert text.index("/* ---- closest-point queries") < text.index("/* ---- K-nearest queries")
    for word in ("k < R * R", "(k, kind, primitive)", "a sphere comes before a triangle", "min(total, K)", "point-major", "_reserved[0]",
                 "4194304 / K", "rt_read_bvh_order", '"closest_count"', "rt_multi_closest_points", "rt_closest_points_device"):
        assert word in section, word
    design = open(f"{ROOT}/DESIGN.md").read()
    assert "### K-nearest queries" in design and "k_nearest" in design and "K-th key" in design


def test_the_surface_is_unchanged(rtx):
    assert len(rtx._cabi.SYMBOLS) == 115
    assert not any("nearest" in s or "overlap" in s for s in rtx._cabi.SYMBOLS)
    assert hasattr(rtx.RayTracingManager, "OverlapSphere")
    # the compiled host: RayTracingManager::OverlapSphere and its C entry, which refuses bad arguments before it touches a device.  (The
    # Python window CppScene gets no method: its public surface is a recorded one, tests/golden/cabi_surface.json)
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "OverlapSphere(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    L = rtx.host_cpp_binding.load_host_library()
    import ctypes
    assert L.rth_overlap_sphere(None, None, 0, None, ctypes.c_float(1.0), 0, None, None) == -1 and b"rth_overlap_sphere" in L.rth_last_error()
    cs = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs", "RtNearest.cs")).read()
    assert "struct" not in cs and "static class RtNearest" in cs and '"closest_k"' in cs and '"closest_all"' in cs


def test_nearest_py_refuses_bad_input_before_any_c_call(rtx):
    class Untouchable(rtx.Tracer):
        def __init__(self):
            pass

        def set_option(self, *a):
            raise AssertionError("a C call")
        closest_points = set_option
    tr = Untouchable()
    pts = np.zeros(4, rtx.RAY)
    for bad_points, radius in ((np.zeros((4, 7), np.float32), 1.0), (np.zeros(4, np.float64), 1.0), (pts, np.ones(3)), (pts, np.ones((4, 1)))):
        with pytest.raises(ValueError):
            rtx.nearest.nearest_k(tr, bad_points, 4, radius)
        with pytest.raises(ValueError):
            rtx.nearest.overlap_count(tr, bad_points, radius)
    for k in (0, 9, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            rtx.nearest.nearest_k(tr, pts, k)
    for fn, args in ((rtx.nearest.nearest_k, (pts, 4)), (rtx.nearest.overlap_count, (pts, 1.0))):
        with pytest.raises(TypeError):
            fn(object(), *args)
    with pytest.raises(AssertionError, match="a C call"):      # (good input does reach the tracer)
        rtx.nearest.nearest_k(tr, pts, 4, 1.0)
    q = rtx.nearest._with_radius(pts, [1.0, 2.0, 0.5, 4.0])
    assert (pts["tMax"] == 0).all() and np.array_equal(q["tMax"], np.float32([1, 2, 0.5, 4]))


def test_closest_all_is_put_back_when_restoring_closest_k_fails(rtx):
    lib = cabi_record.Recorder(rtx._cabi.PARAMS.itemsize)
    lib.returns["rt_set_option"] = lambda ctx, name, value: -2 if (name, value) == (b"closest_k", 1) else 0
    t = object.__new__(rtx._cabi.Tracer)
    t._lib, t._ctx = lib, cabi_record.CTX
    with pytest.raises(rtx.RtError):
        rtx.nearest.nearest_k(t, np.zeros(4, rtx.RAY), 3, 1.0, count_all=True)
    options = [(e["args"][1], e["args"][2]) for e in lib.log if e["call"] == "rt_set_option"]
    assert options == [("bytes:closest_k", 3), ("bytes:closest_all", 1), ("bytes:closest_k", 1), ("bytes:closest_all", 0)]
    assert [e["call"] for e in lib.log].index("rt_closest_points") == 2


def test_the_handle_remembers_closest_k(rtx):
    class Quiet(rtx.Tracer):
        def __init__(self):
            self._lib, self._handle = None, None

        def _check(self, rc, what):
            pass
    import types
    tr = Quiet()
    tr._lib = types.SimpleNamespace(rt_set_option=lambda *a: 0)
    assert tr._closest_k == 1 and rtx.MultiTracer._closest_k == 1      # (a class default: there before any set_option)
    tr.set_option("closest_k", 5)
    assert tr._closest_k == 5
    tr.set_option("closest_all", 1)
    assert tr._closest_k == 5


def test_nearest_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_nearest" not in k[".name"]:
                continue
            names[k[".name"]] = k[".vgpr_count"]
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_nearest VGPRs:", names)
    assert len(names) == 4, sorted(names)           # f16 / f32 nodes x plain / counting


# ---- the oracle against the existing checker, and the prefix property ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(rtx):
    """name -> (spheres, triangles, meshinfo, the GPU tests' batch), each made once"""
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            p = nc.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
            p.setflags(write=False)
            cache[name] = (s, t, m, p)
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_closest_point_checker_and_the_prefix_property(rtx, batches, name):
    s, t, m, p = batches(name)
    default = cc.oracle_closest(rtx, s, t, m, p)
    one_ = nc.oracle_nearest(rtx, s, t, m, p, 1, 0)
    assert one_.shape == (len(p), 1)
    cc.assert_same_records(rtx, one_[:, 0], default, f"{name}: K = 1, all = 0 is today's call")      # (_reserved 0 included)
    totals = np.zeros(len(p), np.int32)
    full = nc.oracle_nearest(rtx, s, t, m, p, 8, 0, totals=totals)
    full_all = nc.oracle_nearest(rtx, s, t, m, p, 8, 1)
    assert np.array_equal(counts(full_all), np.repeat(totals[:, None], 8, 1))
    for k in range(1, 9):
        for count_all in (0, 1):
            r = nc.oracle_nearest(rtx, s, t, m, p, k, count_all)
            if (k, count_all) != (1, 0):
                nc.assert_first_is_the_default(rtx, r, default, f"{name} K {k} all {count_all}")
                want_count = totals if count_all else np.minimum(totals, k)
                assert np.array_equal(counts(r), np.repeat(want_count[:, None], k, 1)), (name, k, count_all)
                assert (r["_reserved"][..., 1] == 0).all()
            # the records of K = j are the first j of K = 8, the count apart
            a, b = nc.words(rtx, r).copy(), nc.words(rtx, full[:, :k]).copy()
            a[..., nc.COUNT_WORD] = b[..., nc.COUNT_WORD] = 0
            assert np.array_equal(a, b), (name, k, count_all)
    # ascending distances (the order at equal KEYS is the hand cases' business: two keys can round to one dst)
    d = full["dst"]
    with np.errstate(invalid="ignore"):
        assert (np.diff(d, axis=1)[np.isfinite(d[:, 1:])] >= 0).all()


def test_the_batches_make_evictions_and_ties_at_the_kth_key(rtx, batches):
    """by construction: vertex_tie_points sit above vertices of a power-of-two grid with R = four cells, so more than eight candidates lie
    within R and the six triangles of an inner vertex tie bit for bit — the 4th and 5th keys of the full sort are equal"""
    s, t, m, p = batches("plane")
    totals, ties = np.zeros(len(p), np.int32), np.zeros(len(p), np.int32)
    nc.oracle_nearest(rtx, s, t, m, p, 4, 0, totals=totals, kth_ties=ties)
    print(f"plane batch: {len(p)} points, {int((totals > 8).sum())} with more than 8 candidates, {int(ties.sum())} with the 4th and 5th key equal")
    assert (totals > 8).sum() >= 100 and ties.sum() >= 50
    s, t, m = nc.tie_plane(rtx)
    q = nc.vertex_tie_points(rtx, s, t, m)
    totals, ties = np.zeros(len(q), np.int32), np.zeros(len(q), np.int32)
    nc.oracle_nearest(rtx, s, t, m, q, 4, 0, totals=totals, kth_ties=ties)
    assert (totals > 8).sum() >= 100 and ties.sum() >= 50, (int((totals > 8).sum()), int(ties.sum()))


# ---- hand cases on dyadic numbers -----------------------------------------------------------------------------------------------------------
def _plane44(rtx, chunks=None):
    s, t, m = plane(rtx, 4, 4)                      # spacing 2.0: A + (B - A) == B exactly
    if chunks is not None:
        m = np.zeros(len(chunks), rtx.MESHINFO)
        for i, (first, count) in enumerate(chunks):
            m["firstTriangleIndex"][i], m["numTriangles"][i] = first, count
    return s, t, m


SIX = [10, 11, 13, 18, 20, 21]                      # the triangles of plane(rtx, 4, 4) that meet at vertex (4, 4, 0)


def test_six_triangles_tie_above_an_inner_vertex(rtx):
    assert nc.around_vertex(4, 2, 2) == SIX
    for chunks, chunk_of in ((None, lambda prim: 0), ([(16, 16), (0, 16)], lambda prim: 0 if prim >= 16 else 1)):
        sc = _plane44(rtx, chunks)
        r = near(rtx, sc, (4, 4, 1), 1.5, 8)
        assert list(r["primitive"]) == SIX + [-1, -1] and (r["kind"][:6] == 2).all() and (r["kind"][6:] == 0).all(), r
        assert (r["dst"][:6] == 1.0).all() and np.isposinf(r["dst"][6:]).all() and (counts(r) == 6).all()
        assert (r["point"][:6] == (4, 4, 0)).all() and (r["side"][:6] == 1).all() and (r["normal"][:6] == (0, 0, 1)).all()
        assert [chunk_of(int(x)) for x in r["primitive"][:6]] == list(r["chunk"][:6])
        # (u, v) name the vertex in each triangle's own frame
        for rec in r[:6]:
            A, B, C = (sc[1][k][rec["primitive"]] for k in ("posA", "posB", "posC"))
            assert tuple(A + (B - A) * rec["u"] + (C - A) * rec["v"]) == (4, 4, 0)
        r4 = near(rtx, sc, (4, 4, 1), 1.5, 4)
        assert list(r4["primitive"]) == SIX[:4] and (counts(r4) == 4).all()
        assert (counts(near(rtx, sc, (4, 4, 1), 1.5, 4, 1)) == 6).all() and (counts(near(rtx, sc, (4, 4, 1), 1.5, 1, 1)) == 6).all()
        # unbounded: the six first, then the two triangles of the four cells that do not touch the vertex (key 1 + 2)
        r8 = near(rtx, sc, (4, 4, 1), np.inf, 8)
        assert list(r8["primitive"][:6]) == SIX and sorted(r8["primitive"][6:]) == [12, 19] and (r8["dst"][6:] == np.sqrt(np.float32(3))).all()
        assert (counts(r8) == 8).all() and (counts(near(rtx, sc, (4, 4, 1), np.inf, 8, 1)) == 32).all()


def test_a_sphere_comes_before_a_triangle_at_one_key(rtx):
    sc = scene(rtx, [T0], [((9, 9, 9), 1.0), ((1, 1, 6), 2.0)])         # triangle and sphere 1 at key 4 from (1, 1, 2)
    r = near(rtx, sc, (1, 1, 2), np.inf, 2)
    assert list(r["kind"]) == [1, 2] and list(r["primitive"]) == [1, 0] and (r["dst"] == 2.0).all() and (counts(r) == 2).all()
    r = near(rtx, sc, (1, 1, 2), np.inf, 3, 1)
    assert list(r["kind"]) == [1, 2, 1] and list(r["primitive"]) == [1, 0, 0] and (counts(r) == 3).all()
    # two spheres at one key: the lower index
    r = near(rtx, scene(rtx, spheres=[((0, 0, 4), 2.0), ((0, 0, -4), 2.0)]), (0, 0, 0), np.inf, 2)
    assert list(r["primitive"]) == [0, 1] and (r["dst"] == 2.0).all()


def test_ties_above_a_cubes_corner(rtx):
    sc = scene(rtx, CUBE)
    r = near(rtx, sc, (3, 3, 3), np.inf, 8)
    at_corner = [i for i, tri in enumerate(CUBE) if (2, 2, 2) in tri]
    assert len(at_corner) >= 3
    n = len(at_corner)
    assert list(r["primitive"][:n]) == at_corner and (r["dst"][:n] == np.sqrt(np.float32(3))).all() and (r["point"][:n] == (2, 2, 2)).all()
    assert (r["dst"][n:] > r["dst"][0]).all()
    assert list(near(rtx, sc, (3, 3, 3), np.inf, 3)["primitive"]) == at_corner[:3]


def test_the_radius_is_strict(rtx):
    sc = _plane44(rtx)
    for k, count_all in ((8, 0), (4, 1), (1, 1)):
        r = near(rtx, sc, (4, 4, 1), 1.0, k, count_all)                 # the six keys are 1.0 == R * R: neither listed nor counted
        assert (r["kind"] == 0).all() and (counts(r) == 0).all() and np.isposinf(r["dst"]).all()
        r = near(rtx, sc, (4, 4, 1), np.nextafter(np.float32(1), np.float32(2)), k, count_all)
        assert (r["kind"][:min(k, 6)] == 2).all() and (counts(r) == (6 if count_all else min(k, 6))).all()


def test_points_and_radii_that_are_not_searched(rtx):
    sc = scene(rtx, [T0], [((0, 0, 8), 1.0)])
    for p, R in (((np.nan, 1, 1), np.inf), ((1, np.inf, 1), np.inf), ((1, 1, 2), 0.0), ((1, 1, 2), -1.0), ((1, 1, 2), np.nan)):
        for k, count_all in ((8, 0), (3, 1), (1, 1)):
            r = near(rtx, sc, p, R, k, count_all)
            assert r.shape == (k,) and (r["kind"] == 0).all() and np.isposinf(r["dst"]).all() and (r["primitive"] == -1).all()
            assert (r["chunk"] == -1).all() and (r["mesh"] == -1).all() and (r["side"] == 0).all() and (r["_reserved"] == 0).all()
            assert (r["point"] == 0).all() and (r["normal"] == 0).all() and (r["u"] == 0).all() and (r["v"] == 0).all()


def test_a_closed_form_count(rtx):
    """tie_plane(8): 128 triangles on a grid of spacing 2; the point one unit above the centre vertex (8, 8).  Keys are 1 + d^2, d the
    distance in the plane from the vertex to the triangle: 0 for the six that meet there; sqrt 2 for the two others of the four cells
    around it (their diagonal passes at sqrt 2); 2 for the twelve triangles outside those four cells that touch one of the four points
    (8 +- 2, 8), (8, 8 +- 2) — every other point outside the cells is farther than 2 — three outside the cells at each of the four."""
    sc = nc.tie_plane(rtx, 8)
    for R, want in ((1.0, 0), (1.5, 6), (1.75, 8), (2.0, 8), (2.25, 20), (64.0, 128)):
        for k in (1, 8):
            assert (counts(near(rtx, sc, (8, 8, 1), R, k, 1)) == want).all(), (R, k)


# ---- float64 twin ----------------------------------------------------------------------------------------------------------------------------
def test_checker_against_the_float64_twin(rtx):
    rng = np.random.default_rng(20261)
    cases, worst, counted = 300, 0.0, 0
    for _ in range(cases):
        A, B, C, c, r, p = _random_case(rng, nt=12, ns=3)
        sc = scene(rtx, list(zip(A, B, C)), list(zip(c, r)))
        R = np.float32(rng.uniform(0.3, 1.5))
        dst = nc.twin_sorted_dst(p, R, c, r, A, B, C)
        assert len(dst) == 15
        tol = max(max(cc.dst_tolerance(p, kind, prim, c, r, A, B, C)) for kind, n in ((1, 3), (2, 12)) for prim in range(n))
        got = near(rtx, sc, p, np.inf, 8)
        err = np.abs(got["dst"].astype(np.float64) - dst[:8])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (got["dst"], dst[:8], tol)
        # the count of a bounded search, between the twin's counts on either side of R
        n_all = int(counts(near(rtx, sc, p, R, 3, 1))[0])
        lo, hi = int((dst < float(R) - tol).sum()), int((dst < float(R) + tol).sum())
        assert lo <= n_all <= hi, (n_all, lo, hi)
        assert int(counts(near(rtx, sc, p, R, 3, 0))[0]) == min(n_all, 3)
        counted += n_all
    print(f"twin: {cases} cases, largest |dst - twin| / tolerance {worst:.3f}, {counted / cases:.1f} candidates within R on average")
    assert 2 < counted / cases < 13


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
def _hand_cases(rtx):
    """(scene, point, R, K, all) of the hand cases above"""
    out_of_order = _plane44(rtx, [(16, 16), (0, 16)])
    both = scene(rtx, [T0], [((9, 9, 9), 1.0), ((1, 1, 6), 2.0)])
    return [(_plane44(rtx), (4, 4, 1), 1.0, 8, 0), (_plane44(rtx), (4, 4, 1), 1.5, 4, 1), (out_of_order, (4, 4, 1), 1.5, 4, 0),
            (out_of_order, (4, 4, 1), 1.5, 8, 0), (both, (1, 1, 2), np.inf, 2, 0), (scene(rtx, CUBE), (3, 3, 3), np.inf, 3, 0)]


@pytest.mark.parametrize("mutant", list(nc.MUTANTS))
def test_every_mutant_differs_on_a_hand_case(rtx, mutant):
    caught = [i for i, (sc, p, R, k, a) in enumerate(_hand_cases(rtx))
              if nc.different(rtx, near(rtx, sc, p, R, k, a), near(rtx, sc, p, R, k, a, variant=nc.MUTANTS[mutant]))]
    print(mutant, "differs on hand cases", caught)
    assert caught, mutant
