"""Multi-hit ray queries without a GPU: the checker (tests/hits_oracle.c) is pinned independently of the kernel — by hand-computed cases on
dyadic numbers, by a float64 twin of the definition that sorts everything with numpy, and at K = 1 by the ray queries' own checker
(rq_trace) — and the boundary is checked: sizes, exports, bindings, the four k_multihit instantiations without scratch.

The float64 twin, and the tolerance.  eps = 2^-24.  For a ray (o, d) and a triangle let ao = o - A, P = |eAB| |eAC|, L = max(|eAB|, |eAC|),
det = -dot(d, n).  In the checker's float32 a component of eAB, eAC or ao carries one rounding; a cross product of two such vectors has
per component two products and a difference of rounded inputs: at most 6 eps of the product of the lengths; a dot of two such vectors
three products and two sums: with the inputs' errors at most 16 eps of the product of the lengths.  So |d num| <= 16 eps |ao| P for
num = dot(ao, n), |d det| <= 16 eps |d| P, |d (eAC . dao)| <= 16 eps L |ao| |d|.  The quotient through inv = 1 / det (one rounding) and a
product (one more): |d dst| <= (|d num| + dst |d det|) / |det| + 2 eps dst = 16 eps P (|ao| + dst |d|) / |det| + 2 eps dst, and with |u| <= 1,
|d u| <= 16 eps |d| (L |ao| + P) / |det| + 2 eps; w = 1 - u - v: twice that plus 2 eps.  A sphere: |d b| <= 8 eps |oc| |d| =: Eb,
|d c| <= 8 eps (|oc|^2 + r^2) =: Ec, |d disc| <= 2 |b| Eb + 4 a Ec + 4 eps (b^2 + 4 a |c|) =: Ed, |d sqrt| <= Ed / sqrt(disc) (for
disc >= 4 Ed; a sphere nearer to tangency makes the ray fragile), |d root| <= (Eb + Ed / sqrt(disc)) / (2 a) + 4 eps |root|.
A ray is compared when (1) no candidate is FRAGILE: a triangle whose u, v, w, dst or |det| - 1e-6 lies within its bound of the
acceptance threshold while the other conditions hold, a sphere with 0 <= disc < 4 Ed (or -Ed < disc < 0) or a root within its bound of
0, or any accepted dst within its bound of tMax; and (2) consecutive float64 hits are more than tol apart, tol = twice the largest
|d dst| among the ray's hits (each of two neighbours can move by its own bound).  For such a ray the float32 order is the float64 order,
so kinds, primitives and sides must agree exactly and every dst within its bound.  The share of rays compared is printed and must be
at least half."""
import ctypes
import os
import re

import numpy as np
import pytest

import hits_check as hc
import query_check
from ray_query_helpers import shim  # noqa: F401  (fixture)
from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_trace_hits", "rt_trace_hits_device", "rt_get_hits_info", "rt_multi_trace_hits")
EPS = 2.0 ** -24
INF = np.inf


def scene(rtx, tris=(), spheres=(), chunks=None, bounds=None):
    """(spheres, triangles, meshinfo): triangles as (A, B, C) triples with the normal (0, 0, 1) at every vertex, spheres as (centre,
    radius); one chunk over all triangles unless chunks = [(first, count), ...]; every chunk's box is `bounds` (default: everything)"""
    t = np.zeros(len(tris), rtx.TRIANGLE)
    for i, (A, B, C) in enumerate(tris):
        t["posA"][i], t["posB"][i], t["posC"][i] = A, B, C
    t["normalA"] = t["normalB"] = t["normalC"] = (0.0, 0.0, 1.0)
    s = np.zeros(len(spheres), rtx.SPHERE)
    for i, (c, r) in enumerate(spheres):
        s["position"][i], s["radius"][i] = c, r
    chunks = ([(0, len(tris))] if len(tris) else []) if chunks is None else chunks
    m = np.zeros(len(chunks), rtx.MESHINFO)
    for i, (first, count) in enumerate(chunks):
        m["firstTriangleIndex"][i], m["numTriangles"][i] = first, count
        m["boundsMin"][i], m["boundsMax"][i] = bounds[i] if bounds else ((-64, -64, -64), (64, 64, 64))
    return s, t, m


def cast(rtx, sc, o, d, t_max=INF, K=8, mode=hc.BOTH, count_all=False, intersect=1):
    return hc.oracle_hits(rtx, *sc, hc.make_rays(rtx, [o], [d], t_max), K, mode, count_all, intersect)[0]


def keys(rec):
    """[(dst, kind, primitive, side), ...] of the non-empty records"""
    return [(float(r["dst"]), int(r["kind"]), int(r["primitive"]), int(r["side"])) for r in rec if r["kind"] != 0]


def quad(z, flip=False):
    """two triangles over [0, 4]^2 at height z facing +z (flip: -z)"""
    a, b, c, d = (0, 0, z), (4, 0, z), (4, 4, z), (0, 4, z)
    return [(a, c, b), (a, d, c)] if flip else [(a, b, c), (a, c, d)]


def assert_empty(r, hit_count):
    assert np.isposinf(r["dst"]) and r["kind"] == 0 and r["primitive"] == -1 and r["chunk"] == -1 and r["mesh"] == -1 and r["side"] == 0
    assert (r["hitPoint"] == 0).all() and (r["normal"] == 0).all() and r["u"] == 0 and r["v"] == 0 and r["_reserved"] == 0 and r["hitCount"] == hit_count


# ---- hand-computed cases ---------------------------------------------------------------------------------------------------------------
def test_a_stack_of_quads_in_order_truncated_and_counted(rtx):
    """quads at z = -1, -2, -4, -8 below a ray from (1, 2, 0) along -z: distances 1, 2, 4, 8 on the first triangle of each (the point
    (1, 2) has x < y: the triangle (a, c, d))"""
    sc = scene(rtx, sum((quad(-z) for z in (8.0, 1.0, 4.0, 2.0)), []))           # uploaded out of distance order
    o, d = (1, 2, 0), (0, 0, -1)
    rec = cast(rtx, sc, o, d, mode=hc.FRONT)
    assert keys(rec) == [(1.0, 2, 3, 1), (2.0, 2, 7, 1), (4.0, 2, 5, 1), (8.0, 2, 1, 1)]
    assert all(r["hitCount"] == 4 for r in rec)
    for r in rec[4:]:
        assert_empty(r, 4)
    first = rec[0]
    assert tuple(first["hitPoint"]) == (1, 2, -1) and tuple(first["normal"]) == (0, 0, 1) and first["chunk"] == 0 and first["mesh"] == -1
    assert first["u"] == 0.25 and first["v"] == 0.25          # weights of B = c (4, 4) and C = d (0, 4): (1, 2) = a/4 + c/4 + d/4 ... u c + v d = (1, 2)
    # a direction of length 2 halves every dst
    assert [k[0] for k in keys(cast(rtx, sc, o, (0, 0, -2), mode=hc.FRONT))] == [0.5, 1.0, 2.0, 4.0]
    # K truncation and both countAll values
    for K in (1, 2, 3):
        cut = cast(rtx, sc, o, d, K=K, mode=hc.FRONT)
        assert len(cut) == K and keys(cut) == keys(rec)[:K] and all(r["hitCount"] == K for r in cut)
        assert all(r["hitCount"] == 4 for r in cast(rtx, sc, o, d, K=K, mode=hc.FRONT, count_all=True))
    assert all(r["hitCount"] == 4 for r in cast(rtx, sc, o, d, K=8, mode=hc.FRONT, count_all=True))
    # tMax is strict: exactly a hit's dst drops it, the next float keeps it; countAll counts below tMax only
    assert [k[0] for k in keys(cast(rtx, sc, o, d, t_max=4.0))] == [1.0, 2.0]
    assert [k[0] for k in keys(cast(rtx, sc, o, d, t_max=np.nextafter(np.float32(4), np.float32(5))))] == [1.0, 2.0, 4.0]
    assert cast(rtx, sc, o, d, t_max=4.0, K=1, count_all=True)[0]["hitCount"] == 2
    # from below the quads show their backs: nothing in FRONT mode, all four in BOTH, sides -1, normals not flipped
    up = cast(rtx, sc, (1, 2, -16), (0, 0, 1), mode=hc.BOTH)
    assert keys(up) == [(8.0, 2, 1, -1), (12.0, 2, 5, -1), (14.0, 2, 7, -1), (15.0, 2, 3, -1)] and tuple(up[0]["normal"]) == (0, 0, 1)
    assert up[0]["u"] == 0.25 and up[0]["v"] == 0.25
    assert keys(cast(rtx, sc, (1, 2, -16), (0, 0, 1), mode=hc.FRONT)) == []


def test_sphere_entry_exit_inside_and_tangent(rtx):
    sc = scene(rtx, spheres=[((0, 0, 4), 1.0)])
    rec = cast(rtx, sc, (0, 0, 0), (0, 0, 1))
    assert keys(rec) == [(3.0, 1, 0, 1), (5.0, 1, 0, -1)]
    assert tuple(rec[0]["hitPoint"]) == (0, 0, 3) and tuple(rec[0]["normal"]) == (0, 0, -1) and rec[0]["chunk"] == -1 and rec[0]["u"] == 0
    assert tuple(rec[1]["hitPoint"]) == (0, 0, 5) and tuple(rec[1]["normal"]) == (0, 0, 1)
    assert keys(cast(rtx, sc, (0, 0, 0), (0, 0, 1), mode=hc.FRONT)) == [(3.0, 1, 0, 1)]
    # from inside: the entry root is negative, the exit alone
    assert keys(cast(rtx, sc, (0, 0, 4), (0, 0, 1))) == [(1.0, 1, 0, -1)] and keys(cast(rtx, sc, (0, 0, 4), (0, 0, 1), mode=hc.FRONT)) == []
    # tangent: disc == 0, both roots 4, front first
    tan = cast(rtx, sc, (1, 0, 0), (0, 0, 1))
    assert keys(tan) == [(4.0, 1, 0, 1), (4.0, 1, 0, -1)] and tuple(tan[0]["normal"]) == (1, 0, 0)
    assert keys(cast(rtx, sc, (1, 0, 0), (0, 0, 1), K=1)) == [(4.0, 1, 0, 1)]
    # origin on the surface: dst == 0 counts (and the exit 2 away)
    assert keys(cast(rtx, sc, (0, 0, 3), (0, 0, 1))) == [(0.0, 1, 0, 1), (2.0, 1, 0, -1)]


def test_a_closed_cube_gives_one_front_and_one_back_hit(rtx):
    s, t, m = hc.shells(rtx)
    sc = (s[:0], t[:12], m[:1])                                     # the innermost cube, half 0.25 around (1, 2, 3)
    rec = cast(rtx, sc, (1.0625, 2.125, 0), (0, 0, 1))
    assert [(k[0], k[3]) for k in keys(rec)] == [(2.75, 1), (3.25, -1)]
    assert tuple(rec[0]["normal"]) == (0, 0, -1) and tuple(rec[1]["normal"]) == (0, 0, 1)       # outward both times: not flipped
    inside = cast(rtx, sc, (1, 2.125, 3), (1, 0, 0))
    assert [(k[0], k[3]) for k in keys(inside)] == [(0.25, -1)]
    assert keys(cast(rtx, sc, (1.0625, 2.125, 0), (0, 0, 1), mode=hc.FRONT)) == keys(rec)[:1]


def test_ties_lower_index_first_and_sphere_before_triangle(rtx):
    T = ((0, 0, 0), (4, 0, 0), (0, 4, 0))
    for order in ([T, T], [T, T, T]):
        rec = cast(rtx, scene(rtx, order), (1, 1, 2), (0, 0, -1))
        assert keys(rec) == [(2.0, 2, i, 1) for i in range(len(order))]
    # the uploaded index decides, not the chunk order
    rec = cast(rtx, scene(rtx, [T, T], chunks=[(1, 1), (0, 1)]), (1, 1, 2), (0, 0, -1))
    assert keys(rec) == [(2.0, 2, 0, 1), (2.0, 2, 1, 1)] and [int(r["chunk"]) for r in rec[:2]] == [1, 0]
    assert keys(cast(rtx, scene(rtx, [T, T], chunks=[(1, 1), (0, 1)]), (1, 1, 2), (0, 0, -1), K=1)) == [(2.0, 2, 0, 1)]
    # a sphere entered at dst 2 and a triangle at dst 2: the sphere first, wherever it sits in its buffer
    sc = scene(rtx, [T], [((9, 9, 9), 1.0), ((1, 1, -1), 1.0)])
    assert keys(cast(rtx, sc, (1, 1, 2), (0, 0, -1)))[:2] == [(2.0, 1, 1, 1), (2.0, 2, 0, 1)]
    # a shared edge: both triangles at the same dst, the lower index first
    rec = cast(rtx, scene(rtx, quad(0.0)), (2, 2, 1), (0, 0, -1))
    assert keys(rec) == [(1.0, 2, 0, 1), (1.0, 2, 1, 1)]


def test_zero_distances_and_minus_zero(rtx):
    T = ((0, 0, 0), (4, 0, 0), (0, 4, 0))
    # the origin on the triangle: dot(ao, n) = +0, det > 0: dst = +0
    rec = cast(rtx, scene(rtx, [T]), (1, 1, 0), (0, 0, -1))
    assert keys(rec) == [(0.0, 2, 0, 1)] and not np.signbit(rec[0]["dst"])
    # seen from behind, det < 0: dst = +0 * (1 / det) = -0.0f, which is >= 0 and counts; it ties with a +0.0f of a lower key
    back = cast(rtx, scene(rtx, [T]), (1, 1, 0), (0, 0, 1))
    assert keys(back) == [(0.0, 2, 0, -1)] and np.signbit(back[0]["dst"]) and tuple(back[0]["hitPoint"]) == (1, 1, 0)
    Tb = (T[0], T[2], T[1])                                                 # the same triangle wound the other way: its front looks down
    both = cast(rtx, scene(rtx, [T, Tb]), (1, 1, 0), (0, 0, 1))
    assert [(k[1], k[2], k[3]) for k in keys(both)] == [(2, 0, -1), (2, 1, 1)] and np.signbit(both[0]["dst"]) and not np.signbit(both[1]["dst"])
    both = cast(rtx, scene(rtx, [Tb, T]), (1, 1, 0), (0, 0, 1))
    assert [(k[1], k[2], k[3]) for k in keys(both)] == [(2, 0, 1), (2, 1, -1)]       # -0.0f == 0.0f: the index decides


def test_rays_that_are_not_traced_or_hit_nothing(rtx):
    sc = scene(rtx, quad(-1.0), [((0, 0, -4), 1.0)])
    for t_max in (0.0, -1.0, np.nan):
        for count_all in (False, True):
            rec = cast(rtx, sc, (1, 2, 0), (0, 0, -1), t_max=t_max, K=3, count_all=count_all)
            assert len(rec) == 3
            for r in rec:
                assert_empty(r, 0)
    for o, d in (((np.nan, 2, 0), (0, 0, -1)), ((1, 2, 0), (0, 0, 0)), ((1, 2, 0), (0, np.inf, -1)), ((1, 2, 0), (-0.0, 0, 0))):
        assert keys(cast(rtx, sc, o, d)) == []
    assert keys(hc.oracle_hits(rtx, *scene(rtx), hc.make_rays(rtx, [(0, 0, 0)], [(0, 0, 1)]))[0]) == []
    # a triangle no chunk addresses is no candidate
    assert keys(cast(rtx, scene(rtx, quad(-1.0), chunks=[(1, 1)]), (1, 2, 0), (0, 0, -1))) == [(1.0, 2, 1, 1)]


def test_chunk_boxes_count_in_flat_chunks_mode_only(rtx):
    """the chunk's box lies beside the ray: RayBoundingBox fails, FLAT_CHUNKS drops the triangle, BRUTE keeps it"""
    sc = scene(rtx, quad(-1.0) + quad(-2.0), chunks=[(0, 2), (2, 2)], bounds=[((0, 0, -1), (4, 4, -1)), ((8, 8, -2), (9, 9, -2))])
    assert [k[0] for k in keys(cast(rtx, sc, (1, 2, 0), (0, 0, -1), intersect=rtx.RT_INTERSECT_BRUTE))] == [1.0, 2.0]
    assert [k[0] for k in keys(cast(rtx, sc, (1, 2, 0), (0, 0, -1), intersect=rtx.RT_INTERSECT_FLAT_CHUNKS))] == [1.0]
    assert cast(rtx, sc, (1, 2, 0), (0, 0, -1), K=1, count_all=True, intersect=rtx.RT_INTERSECT_FLAT_CHUNKS)[0]["hitCount"] == 1


def test_the_untruncated_list_is_the_truncated_one_continued(rtx):
    s, t, m = hc.layers(rtx)
    ray = hc.make_rays(rtx, [(1.25, 2.375, 8)], [(0.03125, 0.0625, -1)])       # (it stays inside one cell, off its diagonal)
    full = hc.oracle_all(rtx, s, t, m, ray, hc.BOTH)
    assert len(full) == 12 and (np.diff(full["dst"]) > 0).all() and (full["hitCount"] == 12).all()
    assert [int(x) for x in full["side"]] == [1 if p % 3 != 2 else -1 for p in range(11, -1, -1)]
    for K in (1, 3, 8):
        cut = hc.oracle_hits(rtx, s, t, m, ray, K, hc.BOTH, True)[0]
        assert (cut["hitCount"] == 12).all()
        a, b = cut.copy(), full[:K].copy()
        hc.assert_same_records(rtx, a, b, f"K = {K}")
    assert len(hc.oracle_all(rtx, s, t, m, ray, hc.FRONT)) == 8


# ---- the float64 twin -------------------------------------------------------------------------------------------------------------------
def _bounds64(o, d, t_max, sc, sr, A, B, C):
    """(tol, fragile): the module docstring's bounds for one ray — twice the largest |d dst| among candidates that could count, and whether
    any candidate sits within its bound of an acceptance threshold"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    nd = np.linalg.norm(d)
    worst, fragile = 0.0, False
    if len(sc):
        oc = o - np.asarray(sc, np.float64)
        r = np.asarray(sr, np.float64)
        a, b = d @ d, 2.0 * (oc @ d)
        noc = np.linalg.norm(oc, axis=1)
        c = noc ** 2 - r ** 2
        disc = b * b - 4 * a * c
        Eb, Ec = 8 * EPS * noc * nd, 8 * EPS * (noc ** 2 + r ** 2)
        Ed = 2 * np.abs(b) * Eb + 4 * a * Ec + 4 * EPS * (b * b + 4 * a * np.abs(c))
        fragile |= bool(((disc > -Ed) & (disc < 4 * Ed)).any())
        ok = disc >= 4 * Ed
        sq = np.sqrt(np.where(ok, disc, 1.0))
        for sgn in (-1.0, 1.0):
            root = (-b + sgn * sq) / (2 * a)
            E = (Eb + Ed / sq) / (2 * a) + 4 * EPS * np.abs(root)
            fragile |= bool((ok & (np.abs(root) <= E)).any()) or bool((ok & (np.abs(root - t_max) <= E)).any())
            live = ok & (root >= 0) & (root < t_max)
            if live.any():
                worst = max(worst, float(E[live].max()))
    if len(A):
        A, B, C = (np.asarray(x, np.float64) for x in (A, B, C))
        eAB, eAC = B - A, C - A
        ao = o - A
        nao, lab, lac = np.linalg.norm(ao, axis=1), np.linalg.norm(eAB, axis=1), np.linalg.norm(eAC, axis=1)
        P, L = lab * lac, np.maximum(lab, lac)
        n = np.cross(eAB, eAC)
        det = -(n @ d)
        adet = np.abs(det)
        Edet = 16 * EPS * nd * P
        near_det = np.abs(adet - 1e-6) <= Edet
        safe = np.where(adet > 0, adet, 1.0)
        q = (ao * n).sum(1) / np.where(det != 0, det, 1.0)
        dao = np.cross(ao, d)
        u = (eAC * dao).sum(1) / np.where(det != 0, det, 1.0)
        v = -(eAB * dao).sum(1) / np.where(det != 0, det, 1.0)
        w = 1 - u - v
        Eq = 16 * EPS * P * (nao + np.abs(q) * nd) / safe + 2 * EPS * np.abs(q)
        Eu = 16 * EPS * nd * (L * nao + P) / safe + 2 * EPS
        Ew = 2 * Eu + 2 * EPS
        cand = adet >= 1e-6 - Edet
        almost = cand & (q >= -Eq) & (u >= -Eu) & (v >= -Eu) & (w >= -Ew)
        edge = almost & ((np.abs(q) <= Eq) | (np.abs(u) <= Eu) | (np.abs(v) <= Eu) | (np.abs(w) <= Ew) | near_det | (np.abs(q - t_max) <= Eq))
        fragile |= bool(edge.any())
        live = almost & (q < t_max)
        if live.any():
            worst = max(worst, float(Eq[live].max()))
    return 2 * worst, fragile


def _random_case(rng, nt=10, ns=3):
    A = rng.uniform(-2, 2, (nt, 3))
    B, C = A + rng.uniform(-2, 2, (nt, 3)), A + rng.uniform(-2, 2, (nt, 3))
    c, r = rng.uniform(-2, 2, (ns, 3)), rng.uniform(0.25, 1.5, ns)
    o = rng.uniform(-4, 4, 3)
    d = (rng.uniform(-1, 1, 3) - o) * rng.uniform(0.25, 2.0)
    return tuple(x.astype(np.float32) for x in (A, B, C, c, r, o, d))


@pytest.mark.parametrize("mode", [hc.FRONT, hc.BOTH])
def test_checker_against_the_float64_twin(rtx, mode):
    rng = np.random.default_rng(20261 + mode)
    cases, compared, hits, worst = 1500, 0, 0, 0.0
    for k in range(cases):
        A, B, C, c, r, o, d = _random_case(rng)
        t_max = np.float32(INF if k % 3 else rng.uniform(2.0, 6.0))
        sc = scene(rtx, list(zip(A, B, C)), list(zip(c, r)))
        ray = hc.make_rays(rtx, [o], [d], t_max)
        got = hc.oracle_all(rtx, *sc, ray, mode, rtx.RT_INTERSECT_BRUTE)
        dst, kind, prim, side = hc.twin64(o, d, t_max, c, r, A, B, C, mode == hc.BOTH)
        tol, fragile = _bounds64(o, d, float(t_max), c, r, A, B, C)
        if fragile or (len(dst) > 1 and np.diff(dst).min() <= tol):
            continue
        compared += 1
        hits += len(dst)
        assert len(got) == len(dst), (k, got, dst)
        assert [int(x) for x in got["kind"]] == list(kind) and [int(x) for x in got["primitive"]] == list(prim) and [int(x) for x in got["side"]] == list(side), (k, got, kind, prim, side)
        if len(dst):
            err = float(np.abs(got["dst"].astype(np.float64) - dst).max())
            worst = max(worst, err)
            assert err <= tol / 2, (k, err, tol)
            for K in (1, 3):
                cut = hc.oracle_hits(rtx, *sc, ray, K, mode, False, rtx.RT_INTERSECT_BRUTE)[0]
                assert [int(x) for x in cut["primitive"][:min(K, len(dst))]] == list(prim[:K])
    print(f"twin, mode {mode}: {compared} of {cases} rays compared, {hits} hits, largest |dst - twin| {worst:.3e}")
    assert compared >= cases // 2 and hits >= cases // 2             # (and the rays do hit things)


# ---- K = 1 against the ray queries' checker, on the batches the GPU tests trace ---------------------------------------------------------
@pytest.fixture(scope="module")
def batches(rtx):
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = hc.buffers_of(rtx, name)
            cache[name] = (s, t, m, hc.batch_of(rtx, s, t, m))
        return cache[name]
    return get


SHARED = ("dst", "hitPoint", "normal", "kind", "primitive", "chunk", "mesh", "u", "v")


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("name", hc.SCENES)
def test_k1_front_is_rq_trace_and_tie_rays_stay_under_the_cap(rtx, shim, batches, name, intersect):  # noqa: F811
    s, t, m, rays = batches(name)
    want = query_check.oracle_hits(rtx, shim, s, t, m, intersect, rays)
    cand = query_check.oracle_candidates(rtx, shim, s, t, m, intersect, rays)
    got = hc.oracle_hits(rtx, s, t, m, rays, 1, hc.FRONT, False, intersect)[:, 0]
    assert ((got["hitCount"] > 0) == (want["kind"] != 0)).all()               # every ray, ties included
    tied = cand > 1
    print(f"{name}, intersect {intersect}: {len(rays)} rays, {int((want['kind'] != 0).sum())} hit, {int(tied.sum())} ties at the closest dst")
    assert tied.sum() <= len(rays) // 50, (name, int(tied.sum()), len(rays))
    clear = cand == 1
    for f in SHARED:
        a, b = got[f][clear], want[f][clear]
        assert a.tobytes() == b.tobytes(), (name, f, np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:5])
    assert (got["side"][clear] == 1).all() and (got["kind"][cand == 0] == 0).all()
    # the batch does what the GPU tests need of it
    deep = hc.oracle_hits(rtx, s, t, m, rays, 8, hc.BOTH, True, intersect)
    if name == "layers":
        assert (deep[:, 0]["hitCount"] > 8).sum() > 100                         # evictions happen
    if name == "shells":
        assert (deep["side"] == -1).sum() > 1000 and (deep[:, 0]["hitCount"] > 8).sum() > 100


# ---- boundary ---------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert len(rtx._cabi.SYMBOLS) == 115
    for cls in (rtx.Tracer, rtx.MultiTracer):
        assert hasattr(cls, "trace_hits")
    assert hasattr(rtx.Tracer, "trace_hits_device") and hasattr(rtx.Tracer, "hits_info")
    assert hasattr(rtx.RayTracingManager, "RaycastAll")
    assert hasattr(rtx.host_cpp_binding.CppScene, "raycast_all")
    text = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert '"hits_slice"' in text
    assert re.search(r"RT_HITS_FRONT\s*=\s*0\s*,\s*RT_HITS_BOTH\s*=\s*1", header) and re.search(r"#define\s+RT_HITS_MAX\s+8\b", header)
    assert re.search(r"#define\s+RT_HITS_DEFAULT_MAX\s+4\b", header)
    assert (rtx.HITS_FRONT, rtx.HITS_BOTH, rtx.HITS_MAX, rtx.HITS_DEFAULT_MAX) == (0, 1, 8, 4)
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    table = (("rt_hits_params", rtx.HITS_PARAMS, 32), ("rt_multihit", rtx.MULTIHIT, 64), ("rt_hits_info", rtx.HITS_INFO, 32))
    header = _header()
    for name, dt, size in table:
        assert lib.rt_sizeof(name.encode()) == size == dt.itemsize, name
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)
    assert rtx.MULTIHIT.names == ("dst", "hitPoint", "normal", "kind", "primitive", "chunk", "mesh", "u", "v", "side", "hitCount", "_reserved")
    assert rtx.HITS_PARAMS.names == ("maxHits", "mode", "countAll", "_reserved")
    assert rtx.HITS_INFO.names == ("calls", "lastMaxHits", "lastMode", "lastCountAll", "lastKernelMs", "totalKernelMs")
    # the fields rt_multihit shares with rt_hit sit where rt_hit has them
    for f in SHARED:
        assert rtx.MULTIHIT.fields[f][1] == rtx.HIT.fields[f][1], f

    class CHit(ctypes.Structure):
        _fields_ = [("dst", ctypes.c_float), ("hitPoint", ctypes.c_float * 3), ("normal", ctypes.c_float * 3), ("kind", ctypes.c_int32),
                    ("primitive", ctypes.c_int32), ("chunk", ctypes.c_int32), ("mesh", ctypes.c_int32), ("u", ctypes.c_float),
                    ("v", ctypes.c_float), ("side", ctypes.c_int32), ("hitCount", ctypes.c_int32), ("_reserved", ctypes.c_int32)]

    class CInfo(ctypes.Structure):
        _fields_ = [("calls", ctypes.c_int32), ("lastMaxHits", ctypes.c_int32), ("lastMode", ctypes.c_int32), ("lastCountAll", ctypes.c_int32),
                    ("lastKernelMs", ctypes.c_double), ("totalKernelMs", ctypes.c_double)]
    for cs, dt in ((CHit, rtx.MULTIHIT), (CInfo, rtx.HITS_INFO)):
        assert ctypes.sizeof(cs) == dt.itemsize
        for f, _ in cs._fields_:
            assert getattr(cs, f).offset == dt.fields[f][1], f


def test_csharp_hits_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtHits.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtHitsParams": ("rt_hits_params", rtx.HITS_PARAMS), "RtMultiHit": ("rt_multihit", rtx.MULTIHIT), "RtHitsInfo": ("rt_hits_info", rtx.HITS_INFO)}
    assert set(structs) == set(pairs)
    for cs_name, (c_name, dt) in pairs.items():
        rows, size, _ = _layout(structs, cs_name)
        assert size == lib.rt_sizeof(c_name.encode()) == dt.itemsize, (cs_name, size)
        assert [r[0] for r in rows] == list(dt.names), (cs_name, rows)
        for field, off, nbytes in rows:
            assert off == dt.fields[field][1] and nbytes == dt.fields[field][0].itemsize, (cs_name, field, off, nbytes)


def test_csharp_backend_and_compiled_host_reach_the_entry_points():
    native, backend = open(os.path.join(CS, "RtNative.cs")).read(), open(os.path.join(CS, "RtBackend.cs")).read()
    sig = {"rt_trace_hits": r"IntPtr ctx, \[In\] RtRay\[\] rays, int n, \[In\] RtHitsParams\[\] p, \[Out\] RtMultiHit\[\] result",
           "rt_trace_hits_device": r"IntPtr ctx, IntPtr rays, int n, \[In\] RtHitsParams\[\] p, IntPtr result",
           "rt_get_hits_info": r"IntPtr ctx, out RtHitsInfo info",
           "rt_multi_trace_hits": r"IntPtr multi, \[In\] RtRay\[\] rays, int n, \[In\] RtHitsParams\[\] p, \[Out\] RtMultiHit\[\] result"}
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(" + sig[name] + r"\)", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    assert {"rt_trace_hits", "rt_multi_trace_hits"} <= used
    assert re.search(r"public\s+RtMultiHit\[\]\s+RaycastAll\s*\(\s*Vector3\s+origin\s*,\s*Vector3\s+direction", backend)
    for name in ("rt_hits_params", "rt_multihit", "rt_hits_info"):
        assert '"' + name + '"' in native, name                               # VerifyLayout
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "RaycastAll(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    assert "rth_raycast_all" in open(os.path.join(host, "rt_host_c.cpp")).read()


def test_the_compiled_host_refuses_bad_arguments_before_it_touches_a_device(rtx):
    L = rtx.host_cpp_binding.load_host_library()
    assert L.rth_raycast_all(None, None, 0, None, None, 0.0, 0, 0, None) == -1 and b"rth_raycast_all" in L.rth_last_error()


def test_multihit_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_multihit" not in k[".name"]:
                continue
            names[k[".name"]] = k[".vgpr_count"]
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_multihit VGPRs:", names)
    assert len(names) == 4, sorted(names)           # f16 / f32 nodes x front / both sides
