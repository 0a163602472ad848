"""Sphere casts without a GPU: the header documents the option and the definition, sweep.py refuses bad input before any C call, the
symbol count is unchanged, and the checker (tests/sweep_oracle.c) is pinned independently of the kernel — against analytic cases on
power-of-two coordinates and against a float64 twin written from the header's text — on the very batches the GPU tests use.

The twin (sweep_check.twin64) lists every candidate of a ray in float64.  For every traced ray of the aimed and the overlapping
class (624 of a batch's 710):
    no phantom   the checker's contact (kind, primitive, feature) is one of the twin's candidates, and its dst lies within TWIN_BOUND of
                 that candidate's time, relative to the distance travelled plus the radius: (|dt| * |d|) / (t * |d| + r);
    not early    the checker's dst is not below the twin's first contact by more than the same bound;
    same winner  the checker's contact is the twin's first one (or the same contact point through a neighbouring triangle: the exact
                 tie of a shared edge or vertex), and a miss is the twin's miss.  Left out, at most 2 % of the rays examined: only the
                 cases whose two best candidates lie closer than TWIN_BOUND (measured: at most 8 of 624).
TWIN_BOUND is the largest difference measured over the six batches, 4.1e-5, times four (profiles/sweep_twin_error.txt).  With the guard
at first r * (1 + 2^-10) up to 10 rays of a batch were late or missed: the quadratics' float32 error, about 2^-25 * (|o - P| / r)^2 of r,
exceeded it at 200 radii.  At r * (1 + 2^-6) none is.
The 64 rays parallel to an edge at offset exactly r are tangent by construction: whether they touch is decided by the last bit — of
float32 in the checker, of float64 in the twin — so neither twin candidates nor times can be compared (the ball of radius g, for which
a twin would be decisive, starts overlapping the edge and reports nothing).  What is asserted for them is the physical half of "no
phantom": at the reported centre the float64 distance to the scene is at most g.  How early they are against the twin is printed.
The 16 rays from 1e4 extents away see their balls from 1e4 to 1e6 radii off: 2^-25 * (|o - P| / r)^2 is 3 to 3e4, no guard constant
covers it, and neither winner nor time is compared with the twin (include/rt.h "sphere casts", limits).  Their triangle contacts get
the physical half of "no phantom" too: at the float32 centre the float64 distance to the named triangle is at most g."""
import re

import numpy as np
import pytest

import closest_check as cc
import sweep_check as sc
from test_closest_cpu import scene
from test_gpu_closest import buffers_of
from test_kernarg_layout_cpu import ROOT

NAMES = ("one", "two", "plane", "spheres", "mixed", "Knight")
TWIN_BOUND = 4 * 4.1e-5         # profiles/sweep_twin_error.txt


def one(rtx, sc_, o, d, r, t_max=np.inf):
    hit, occ = sc.oracle_cast(rtx, *sc_, sc.rays_of(rtx, [o], [d], r, t_max))
    assert occ[0] == (hit["kind"][0] != 0)
    return hit[0]


T = ((-8, -8, 0), (8, -8, 0), (0, 8, 0))            # normal +z
CUBE = [((0, 0, 0), (2, 0, 0), (2, 2, 0)), ((0, 0, 0), (2, 2, 0), (0, 2, 0)), ((0, 0, 2), (2, 2, 2), (2, 0, 2)), ((0, 0, 2), (0, 2, 2), (2, 2, 2)),
        ((0, 0, 0), (0, 0, 2), (2, 0, 2)), ((0, 0, 0), (2, 0, 2), (2, 0, 0)), ((0, 2, 0), (2, 2, 2), (0, 2, 2)), ((0, 2, 0), (2, 2, 0), (2, 2, 2)),
        ((0, 0, 0), (0, 2, 2), (0, 0, 2)), ((0, 0, 0), (0, 2, 0), (0, 2, 2)), ((2, 0, 0), (2, 0, 2), (2, 2, 2)), ((2, 0, 0), (2, 2, 2), (2, 2, 0))]


def test_the_header_documents_the_option_and_the_section():
    text = open(f"{ROOT}/include/rt.h").read()
    options = text[text.index("int rt_set_option") - 12000:text.index("int rt_set_option")]
    assert '"sweep"' in options and "sphere casts" in options
    section = text[text.index("/* ---- sphere casts"):text.index("/* ---- radiance queries")]
    for word in ("_reserved", "intersectMode plays no part", "g = r * (1 + 2^-6)", "qa = ee * dd - nd * nd", "CONTACT normal", "feature code",
                 "rt_read_bvh_order", "float spacing"):
        assert word in section, word
    design = open(f"{ROOT}/DESIGN.md").read()
    assert "### Sphere casts" in design and "sweep_node_step" in design


def test_the_surface_is_unchanged(rtx):
    assert len(rtx._cabi.SYMBOLS) == 115
    assert not any("sweep" in s or "sphere_cast" in s for s in rtx._cabi.SYMBOLS)


def test_sweep_py_refuses_bad_input_before_any_c_call(rtx):
    class Untouchable(rtx.Tracer):
        def __init__(self):
            pass

        def set_option(self, *a):
            raise AssertionError("a C call")
        trace_rays = occluded = set_option
    tr = Untouchable()
    rays = np.zeros(4, rtx.RAY)
    for fn in (rtx.sweep.sphere_cast, rtx.sweep.sphere_check):
        for bad_rays, radius in ((np.zeros((4, 7), np.float32), 1.0), (np.zeros(4, np.float64), 1.0), (rays, np.ones(3)), (rays, np.ones((4, 1)))):
            with pytest.raises(ValueError):
                fn(tr, bad_rays, radius)
        with pytest.raises(TypeError):
            fn(object(), rays, 1.0)
    r = rtx.sweep._with_radius(rays, [1.0, 2.0, 0.5, 4.0])
    assert (rays["_reserved"] == 0).all() and np.array_equal(sc.radii_of(r), np.float32([1, 2, 0.5, 4]))


def test_a_ball_dropped_on_a_face_from_the_front_and_from_behind(rtx):
    s = scene(rtx, [T])
    for h, r, dz in ((4.0, 1.0, -2.0), (16.0, 0.5, -0.25), (3.0, 2.0, -1.0)):
        hit = one(rtx, s, (1, -1, h), (0, 0, dz), r)
        assert hit["kind"] == 2 and hit["primitive"] == 0 and hit["chunk"] == 0 and hit["mesh"] == -1 and tuple(hit["_reserved"]) == (1, 0, 0)
        assert hit["dst"] == np.float32((h - r) / abs(dz)) and tuple(hit["hitPoint"]) == (1, -1, 0) and tuple(hit["normal"]) == (0, 0, 1)
        back = one(rtx, s, (1, -1, -h), (0, 0, -dz), r)
        assert tuple(back["_reserved"]) == (2, 0, 0) and back["dst"] == hit["dst"] and tuple(back["normal"]) == (0, 0, -1)
        assert back["u"] == hit["u"] and back["v"] == hit["v"] and tuple(back["hitPoint"]) == (1, -1, 0)
    # an oblique drop: dst = (h - r) / |d . N| all the same
    hit = one(rtx, s, (-2, 0, 4), (1, 0, -2), 1.0)
    assert hit["dst"] == 1.5 and tuple(hit["hitPoint"]) == (-0.5, 0, 0) and tuple(hit["_reserved"]) == (1, 0, 0)


def test_a_ball_onto_a_cubes_edge_and_corner(rtx):
    s = scene(rtx, CUBE)
    edge = one(rtx, s, (-3, -3, 1), (1, 1, 0), 1.0)
    assert edge["kind"] == 2 and edge["_reserved"][0] in (3, 4, 5)
    assert abs(edge["dst"] - (3 - np.sqrt(0.5))) < 1e-6 and np.allclose(edge["hitPoint"], (0, 0, 1), atol=1e-6)
    assert np.allclose(edge["normal"], (-np.sqrt(0.5), -np.sqrt(0.5), 0), atol=1e-6)
    corner = one(rtx, s, (-3, -3, -3), (1, 1, 1), 1.0)
    assert corner["_reserved"][0] in (6, 7, 8) and tuple(corner["hitPoint"]) == (0, 0, 0) and corner["primitive"] == 0
    assert abs(corner["dst"] - (3 - np.sqrt(1 / 3))) < 1e-6 and np.allclose(corner["normal"], -np.sqrt(1 / 3), atol=1e-6)
    assert (corner["u"], corner["v"]) == (0, 0)
    # through two chunks listed out of order the lower uploaded index still wins the tie at the corner
    s2 = scene(rtx, CUBE, chunks=[(6, 6), (0, 6)])
    assert one(rtx, s2, (-3, -3, -3), (1, 1, 1), 1.0)["primitive"] == 0


def test_a_ball_that_starts_overlapping_and_the_strict_tmax(rtx):
    s = scene(rtx, [T], [((0, 0, -20), 1.0)])
    assert one(rtx, s, (0, 0, 0.5), (0, 0, -1), 1.0)["kind"] == 1          # through the triangle it overlaps, onto the sphere behind
    assert one(rtx, s, (0, 0, -18.5), (0, 0, -1), 1.0)["kind"] == 0        # overlapping the sphere: not reported either
    assert one(rtx, s, (0, 0, 4), (0, 0, -2), 1.0, 1.5)["kind"] == 0 and one(rtx, s, (0, 0, 4), (0, 0, -2), 1.0, np.nextafter(np.float32(1.5), np.float32(2)))["kind"] == 2
    miss = one(rtx, s, (0, 0, 4), (0, 0, 2), 1.0)
    assert np.isposinf(miss["dst"]) and miss["primitive"] == -1 and miss["chunk"] == -1 and miss["mesh"] == -1 and (miss["_reserved"] == 0).all()
    for t_max, r in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (np.inf, 0.0), (np.inf, -1.0), (np.inf, np.nan), (np.inf, np.inf)):
        assert one(rtx, s, (0, 0, 4), (0, 0, -2), r, t_max)["kind"] == 0


def test_a_scene_sphere(rtx):
    s = scene(rtx, [T], [((9, 9, 9), 1.0), ((0, 0, 2), 1.0)])
    hit = one(rtx, s, (0, 0, 8), (0, 0, -1), 1.0)
    assert hit["kind"] == 1 and hit["primitive"] == 1 and hit["dst"] == 4.0 and tuple(hit["hitPoint"]) == (0, 0, 3) and tuple(hit["normal"]) == (0, 0, 1)
    assert hit["chunk"] == -1 and hit["mesh"] == -1 and hit["u"] == 0 and hit["v"] == 0 and (hit["_reserved"] == 0).all()
    # a sphere and a triangle at one dst: the sphere wins
    s = scene(rtx, [T], [((4, 0, 1), 1.0)])
    assert one(rtx, s, (4, 0, 5), (0, 0, -1), 1.0)["kind"] == 1 and one(rtx, s, (-4, 0, 5), (0, 0, -1), 1.0)["kind"] == 2


@pytest.fixture(scope="module")
def batches(rtx):
    out = {}
    for name in NAMES:
        s, t, m = buffers_of(rtx, name)
        rays, cls = sc.batch_of(rtx, s, t, m)
        out[name] = (s, t, m, rays, cls, *sc.oracle_cast(rtx, s, t, m, rays))
    return out


def test_the_batches_hit_and_miss_and_reach_every_feature(rtx, batches):
    for name in NAMES:
        s, t, m, rays, cls, hits, occ = batches[name]
        traced = cls < 4
        share = (hits["kind"][traced] != 0).mean()
        assert 0.25 < share < 0.75, (name, share)
        assert (hits["kind"][~traced] == 0).all() and len(rays) == 710
    fc = sc.feature_class(batches["mixed"][5])
    shares = [(fc == k).sum() / (fc != 0).sum() for k in (1, 2, 3, 4)]
    assert min(shares) >= 0.05, shares


def _scene_distance64(c, s, t):
    """float64 distance from c to the nearest sphere surface or triangle"""
    k = []
    if len(t):
        k.append(np.sqrt(cc._tri_keys64(c, *(t[n].astype(np.float64) for n in ("posA", "posB", "posC"))).min()))
    if len(s):
        k.append(np.abs(np.linalg.norm(c - s["position"].astype(np.float64), axis=1) - s["radius"]).min())
    return min(k)


@pytest.mark.parametrize("name", NAMES)
def test_the_checker_against_the_float64_twin(rtx, batches, name):
    s, t, m, rays, cls, hits, _ = batches[name]
    r = sc.radii_of(rays)
    worst, worst_tangent, first, close, compared, examined = 0.0, 0.0, 0, 0, 0, 0
    for i in np.flatnonzero(cls < 3):
        o, d = rays["origin"][i], rays["direction"][i]
        tt, kind, prim, feat, pt = sc.twin64(o, d, rays["tMax"][i], r[i], s["position"], s["radius"], t["posA"], t["posB"], t["posC"])
        tangent = cls[i] == 1
        examined += not tangent
        if hits["kind"][i] == 0:
            assert tangent or len(tt) == 0, (name, i, "a miss where the twin has a contact", tt[:1])
            continue
        scale = np.linalg.norm(d.astype(np.float64))
        dst = float(hits["dst"][i])
        if len(tt):                                                     # not early (the tangent rays': printed only, see the docstring)
            early = (tt[0] - dst) * scale / (tt[0] * scale + float(r[i]))
            worst, worst_tangent = (worst, max(worst_tangent, early)) if tangent else (max(worst, early), worst_tangent)
        if tangent:
            # no phantom, physically: the ball at the reported centre touches the scene (a triangle by the guard; a sphere by its root)
            c32 = (o + d * hits["dst"][i]).astype(np.float64)
            assert _scene_distance64(c32, s, t) <= float(r[i]) * float(sc.GUARD) * (1 + 1e-4), (name, i)
            continue
        compared += 1
        mine = np.flatnonzero((kind == hits["kind"][i]) & (prim == hits["primitive"][i]) & (feat == hits["_reserved"][i][0]))
        assert len(mine) == 1, (name, i, hits[i])                       # no phantom
        worst = max(worst, abs(dst - tt[mine[0]]) * scale / (tt[mine[0]] * scale + float(r[i])))
        gap = (tt[mine[0]] - tt[0]) * scale / (tt[0] * scale + float(r[i]))
        # the same contact through a neighbouring triangle (a shared edge or vertex: an exact tie, decided by the index) is the winner too
        same = mine[0] == 0 or (gap <= TWIN_BOUND and np.abs(pt[mine[0]] - pt[0]).max() <= 1e-9 * (np.abs(pt[0]).max() + 1))
        first += same
        close += not same and gap <= TWIN_BOUND
        assert same or gap <= TWIN_BOUND, (name, i, "a later contact than the twin's", gap)
    print(f"{name}: {compared} hits compared, largest relative difference {worst:.3g} (tangent rays, early only: {worst_tangent:.3g}); the twin's "
          f"winner in {first} of them, another candidate within the bound of it in {close} of {examined} rays examined")
    assert worst <= TWIN_BOUND, (name, worst)
    assert first + close == compared and close <= 0.02 * examined, (name, close, examined)
    # the rays from 1e4 extents away: a triangle contact is a real one — at the float32 centre the float64 distance to the triangle it
    # names is at most g, by the guard and by nothing the quadratics computed
    far = np.flatnonzero((cls == 3) & (hits["kind"] == 2))
    for i in far:
        c32 = (rays["origin"][i] + rays["direction"][i] * hits["dst"][i]).astype(np.float64)
        tri = t[hits["primitive"][i]:hits["primitive"][i] + 1]
        dist = np.sqrt(cc._tri_keys64(c32, *(tri[n].astype(np.float64) for n in ("posA", "posB", "posC")))[0])
        assert dist <= float(r[i]) * float(sc.GUARD) * (1 + 1e-4), (name, i, dist / float(r[i]))
    assert name == "spheres" or len(far) >= 4, (name, len(far))          # (not vacuous: some of the 16 do hit triangles)
