"""Capsule overlap queries without a GPU: the checker (tests/capsule_oracle.c) pinned independently of the kernel, and the boundary.

(a) Hand cases on dyadic numbers: exact k, s, u, v, side and count.  (b) d = 0 against nearest_oracle.c on the GPU tests' own batches.
(c) A float64 twin by another route: the distance from x(s) to a triangle is convex in s, so golden section over s on the float64
point-triangle distance finds the key with no sub-candidates; keys under a per-primitive tolerance, winners where the twin's two best
are further apart than it.  (d) The one-line mutants, each told apart by these inputs.  (e) The boundary: the kernels in the code
object, capsule.py's refusals and its `finally`, the header, RtCapsule.cs."""
import os
import re

import numpy as np
import pytest

import cabi_record
import capsule_check as kc
import closest_check as cc
import nearest_check as nc
from test_camera_batch_cpu import built_library
from test_gpu_closest import batch_of, buffers_of
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata


def tris_of(rtx, A, B, C):
    t = np.zeros(len(A), rtx.TRIANGLE)
    t["posA"], t["posB"], t["posC"] = A, B, C
    t["normalA"] = t["normalB"] = t["normalC"] = (0, 0, 1)
    return t


def one_chunk(rtx, n):
    m = np.zeros(1, rtx.MESHINFO)
    m["numTriangles"] = n
    return m


def spheres_of(rtx, c, r):
    s = np.zeros(len(c), rtx.SPHERE)
    s["position"], s["radius"] = c, r
    return s


def ask(rtx, s, t, p0, p1, R=np.inf, k=1, a=0, variant=kc.DEFINITION):
    return kc.oracle_capsule(rtx, s, t, one_chunk(rtx, len(t)), kc.segments_of(rtx, [p0], [p1], R), k, a, variant=variant)[0]


# ---- (a) hand cases ---------------------------------------------------------------------------------------------------------------------
def _scene(rtx):
    """the right triangle (0,0,0) (4,0,0) (0,4,0), and the square [0,4]^2 as two triangles sharing the edge (0,0,0)-(4,4,0)"""
    tri = tris_of(rtx, [(0, 0, 0)], [(4, 0, 0)], [(0, 4, 0)])
    two = tris_of(rtx, [(0, 0, 0), (0, 0, 0)], [(4, 0, 0), (4, 4, 0)], [(4, 4, 0), (0, 4, 0)])
    return np.zeros(0, rtx.SPHERE), tri, two


def _expect(r, dst, s, u, v, side, count, point=None):
    assert (float(r["dst"]), float(kc.params(r)), float(r["u"]), float(r["v"]), int(r["side"]), int(kc.counts(r))) == (dst, s, u, v, side, count), r
    if point is not None:
        assert tuple(r["point"]) == point, r


def test_hand_cases_on_dyadic_numbers(rtx):
    none, tri, two = _scene(rtx)
    # parallel to the face at height 2: k = 4, and the tie between the endpoints (and every point between) stays with s = 0
    _expect(ask(rtx, none, tri, (1, 1, 2), (2, 1, 2))[0], 2.0, 0.0, 0.25, 0.25, 1, 1, (1.0, 1.0, 0.0))
    _expect(ask(rtx, none, tri, (2, 1, -2), (1, 1, -2))[0], 2.0, 0.0, 0.5, 0.25, -1, 1, (2.0, 1.0, 0.0))
    # piercing the face: k = 0, side = 0, s = t
    _expect(ask(rtx, none, tri, (1, 1, 2), (1, 1, -2))[0], 0.0, 0.5, 0.25, 0.25, 0, 1, (1.0, 1.0, 0.0))
    _expect(ask(rtx, none, tri, (1, 2, -1), (1, 2, 3))[0], 0.0, 0.25, 0.25, 0.5, 0, 1, (1.0, 2.0, 0.0))
    # ending exactly on the face (t = 1 is accepted) and stopping short of it
    _expect(ask(rtx, none, tri, (1, 1, 2), (1, 1, 0))[0], 0.0, 1.0, 0.25, 0.25, 0, 1)
    _expect(ask(rtx, none, tri, (1, 1, 2), (1, 1, 1))[0], 1.0, 1.0, 0.25, 0.25, 1, 1)
    # beside edge AC (x = 0), both endpoints far: the edge pair, (u, v) = (0, t)
    _expect(ask(rtx, none, tri, (-1, 2, 3), (-1, 2, -3))[0], 1.0, 0.5, 0.0, 0.5, 0, 1, (0.0, 2.0, 0.0))
    _expect(ask(rtx, none, tri, (-1, 1, 4), (-1, 1, -12))[0], 1.0, 0.25, 0.0, 0.25, 0, 1, (0.0, 1.0, 0.0))
    # beside edge BC (x + y = 4): the pair reports (1 - t, t)
    _expect(ask(rtx, none, tri, (3, 3, 2), (3, 3, -2))[0], float(np.sqrt(np.float32(2))), 0.5, 0.5, 0.5, 0, 1, (2.0, 2.0, 0.0))
    # the nearest feature is vertex B = (4, 0, 0): a segment crossing beyond it
    _expect(ask(rtx, none, tri, (5, -3, 0), (5, 1, 0))[0], 1.0, 0.75, 1.0, 0.0, 0, 1, (4.0, 0.0, 0.0))
    _expect(ask(rtx, none, tri, (5, -1, 3), (5, -1, -1))[0], float(np.sqrt(np.float32(2))), 0.75, 1.0, 0.0, 0, 1, (4.0, 0.0, 0.0))
    # over the shared edge of two triangles: both listed at one key, the lower index first
    r = ask(rtx, none, two, (0, 0, 1), (4, 4, 1), k=4)
    assert list(r["kind"]) == [2, 2, 0, 0] and list(r["primitive"]) == [0, 1, -1, -1] and (r["dst"][:2] == 1).all() and (kc.counts(r) == 2).all()
    r = ask(rtx, none, two, (0, 0, 1), (4, 4, 1), k=1, a=1)
    assert list(r["primitive"]) == [0] and (kc.counts(r) == 2).all()
    # strictness at k = R * R: dst 2 is outside R = 2 and inside the next float
    _expect(ask(rtx, none, tri, (1, 1, 2), (2, 1, 2), R=2.0)[0], float("inf"), 0.0, 0.0, 0.0, 0, 0)
    _expect(ask(rtx, none, tri, (1, 1, 2), (2, 1, 2), R=np.nextafter(np.float32(2), np.float32(3)))[0], 2.0, 0.0, 0.25, 0.25, 1, 1)
    # a point (d = 0): the closest-point query
    _expect(ask(rtx, none, tri, (1, 1, 2), (1, 1, 2))[0], 2.0, 0.0, 0.25, 0.25, 1, 1)


def test_piercing_on_inputs_that_are_not_dyadic(rtx):
    """The piercing sub-candidate's key is |x - q|^2 of its own (t, u, v), not a constant: on general floats x and q differ by their
    rounding, so a piercing segment's record carries a dst that is tiny and often not 0, with side = 0 and s = t.  Two pierced faces
    are both listed, in the order of their (tiny) keys and then their indices — they need not tie."""
    rng = np.random.default_rng(20281)
    none = np.zeros(0, rtx.SPHERE)
    positive = 0
    for _ in range(200):
        A, B, C = rng.uniform(-3, 3, (3, 3))
        n = np.cross(B - A, C - A)
        if np.linalg.norm(n) < 1.0:
            continue
        n /= np.linalg.norm(n)
        w = rng.uniform(0.15, 0.4, 2)
        q = A + (B - A) * w[0] + (C - A) * w[1]
        lean = rng.uniform(-0.3, 0.3, 3)
        # where the line meets the second face, in the first face's coordinates: well inside, or the case is not about piercing
        q2 = q + 0.25 * ((n + lean) / (1 + lean @ n) - n)
        uv = np.linalg.lstsq(np.stack([B - A, C - A], 1), q2 - A, rcond=None)[0]
        if min(uv[0], uv[1], 1 - uv.sum()) < 0.05:
            continue
        p0, p1 = q + (n + lean) * rng.uniform(0.5, 2), q - (n + lean) * rng.uniform(0.5, 2)
        t = tris_of(rtx, [A, A + n * 0.25], [B, B + n * 0.25], [C, C + n * 0.25])         # a second face a quarter above the first
        r = ask(rtx, none, t, p0, p1, k=3, a=1)
        assert list(r["kind"]) == [2, 2, 0] and sorted(r["primitive"][:2]) == [0, 1] and (kc.counts(r) == 2).all()
        assert (r["side"][:2] == 0).all() and (r["dst"][:2] < 1e-5).all() and (r["dst"][:2] >= 0).all()
        s = kc.params(r)[:2]
        assert ((s > 0) & (s < 1)).all() and np.abs(r["point"][list(r["primitive"][:2]).index(0)] - q).max() < 1e-5
        assert r["dst"][0] <= r["dst"][1] and (r["dst"][0] < r["dst"][1] or r["primitive"][0] == 0)
        # without the piercing sub-candidate the faces are answered through their edges, far away
        far = ask(rtx, none, t, p0, p1, k=3, a=1, variant=kc.MUTANTS["no piercing"])
        assert (far["dst"][:2] > 1e-3).all()
        positive += int((r["dst"][:2] > 0).sum())
    print("piercing records with dst > 0:", positive)
    assert positive > 50


def test_degenerate_triangles(rtx):
    none = np.zeros(0, rtx.SPHERE)
    # A == B: edge AB is the point A (t = 0), edges AC and BC are the segment (0,0,0)-(4,0,0); the face's det is 0 and never pierces
    seg = tris_of(rtx, [(0, 0, 0)], [(0, 0, 0)], [(4, 0, 0)])
    r = ask(rtx, none, seg, (-1, 1, 1), (3, 1, -3))[0]          # P0 in vertex A's region: key 3; the pairs find s = 1/4 at distance 1
    assert float(r["dst"]) == 1.0 and float(kc.params(r)) == 0.25 and tuple(r["point"]) == (0.0, 0.0, 0.0) and int(kc.counts(r)) == 1
    # beside its middle the closest-point test of P0 gives u = 0 / 0: the running key starts as NaN, nothing is strictly smaller than a
    # NaN, and the triangle does not count — as it does not for the closest-point query of P0
    r = ask(rtx, none, seg, (2, 1, 1), (2, 1, -1))[0]
    assert int(r["kind"]) == 0 and int(kc.counts(r)) == 0
    # a point triangle: every edge is degenerate; the edge branch gives t = 0 and the segment's point nearest to A
    pt = tris_of(rtx, [(1, 1, 0)], [(1, 1, 0)], [(1, 1, 0)])
    keys, par = kc.oracle_keys(rtx, none, pt, kc.segments_of(rtx, [(0, 1, 2)], [(4, 1, 2)]))
    assert float(keys[0, 0]) == 4.0 and float(par[0, 0]) == 0.25


def test_inputs_that_are_not_searched(rtx):
    none, tri, _ = _scene(rtx)
    inf, nan = np.inf, np.nan
    for p0, p1, R in (((1, 1, 2), (2, 1, 2), 0.0), ((1, 1, 2), (2, 1, 2), -1.0), ((1, 1, 2), (2, 1, 2), nan), ((nan, 1, 2), (2, 1, 2), 9.0),
                      ((1, 1, 2), (2, inf, 2), 9.0), ((1, -inf, 2), (2, 1, 2), 9.0), ((1, 1, 2), (2, 1, nan), 9.0)):
        r = ask(rtx, none, tri, p0, p1, R, k=3, a=1)
        assert (r["kind"] == 0).all() and (kc.counts(r) == 0).all() and np.isposinf(r["dst"]).all() and (r["_reserved"][:, 1] == 0).all(), (p0, p1, R)
    g = kc.segments_of(rtx, [(3e38, 0, 0)], d=[(3e38, 0, 0)], radius=inf)                  # P0 and d finite, P1 = +inf
    assert not kc.searched(g)[0] and (kc.oracle_capsule(rtx, none, tri, one_chunk(rtx, 1), g, 1, 0)["kind"] == 0).all()
    assert int(kc.counts(ask(rtx, none, tri, (1, 1, 2), (2, 1, 2), inf))[0]) == 1           # R = +inf is searched


def test_solid_spheres(rtx):
    ball = spheres_of(rtx, [(0, 0, 0)], [2.0])
    none_t = tris_of(rtx, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    r = ask(rtx, ball, none_t, (-4, 3, 0), (4, 3, 0))[0]                                    # passes at distance 3: s = 0.5, dst 1
    assert (float(r["dst"]), float(kc.params(r)), int(r["side"]), tuple(r["point"])) == (1.0, 0.5, 1, (0.0, 2.0, 0.0))
    r = ask(rtx, ball, none_t, (-4, 1, 0), (4, 1, 0))[0]                                    # through the ball: solid, key 0, side -1
    assert (float(r["dst"]), float(kc.params(r)), int(r["side"]), tuple(r["point"])) == (0.0, 0.5, -1, (0.0, 2.0, 0.0))
    r = ask(rtx, ball, none_t, (4, 0, 0), (8, 0, 0))[0]                                     # the endpoint is nearest: clamped to s = 0
    assert (float(r["dst"]), float(kc.params(r)), int(r["side"])) == (2.0, 0.0, 1)
    r = ask(rtx, ball, none_t, (-8, 0, 0), (-3, 0, 0))[0]                                   # clamped to s = 1
    assert (float(r["dst"]), float(kc.params(r))) == (1.0, 1.0)


# ---- (b) d = 0 is the K-nearest query ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "plane", "mixed", "Knight"])
def test_a_point_segment_is_the_k_nearest_query(rtx, name):
    s, t, m = buffers_of(rtx, name)
    q = nc.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
    outside = np.ones(len(q), bool)
    for sp in s:
        outside &= ~(np.linalg.norm(q["origin"].astype(np.float64) - sp["position"], axis=1) < float(sp["radius"]))
    q = q[outside]
    assert len(q) > 500
    for f in nc.FORMS:
        a, b = kc.words(rtx, kc.oracle_capsule(rtx, s, t, m, q, *f)), kc.words(rtx, nc.oracle_nearest(rtx, s, t, m, q, *f))
        assert np.array_equal(a[..., :15], b[..., :15]) and (a[..., 15] == 0).all(), (name, f)


# ---- (c) the float64 twin -----------------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -24


def _tolerance(p0, d, a, b, c):
    """How far the checker's float32 distance from the segment to ONE triangle can lie from the exact one: (below, above).
    below: every sub-candidate's key is the squared distance of two computed points, x within 3 eps |coordinates| of the segment and q
    within 8 eps M of the triangle (closest_check.dst_tolerance's M, taken over both endpoints), so the checker cannot be under the
    minimum by more than 12 eps M.  above: at the true closest pair one of the six sub-candidates applies; its parameters carry
    closest_check.dst_tolerance's region-test error (endpoints) or the pair's quotients' (edges: den = dd ee - b b cancels by
    sin^2 of the angle between d and e, so the error of s0 is bounded by 16 eps / sin^2, that of t0 alike, each at most 1), and the
    distance grows by at most the lengths they move along: (ds |d| + dt L).  The piercing candidate only lowers the minimum."""
    L = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
    far = max(np.linalg.norm(p0 - a), np.linalg.norm(p0 + d - a))
    M = max(np.linalg.norm(p0), np.linalg.norm(p0 + d)) + max(L, far)
    below = 12 * EPS * M
    N2 = float((np.cross(b - a, c - a) ** 2).sum())
    Lp = max(L, far)
    duv = min(118 * EPS * Lp ** 4 / N2 + EPS, 1.0) if N2 > 0 else 1.0
    dl = float(np.linalg.norm(d))
    sin2 = 1.0
    for e in (b - a, c - a, c - b):
        el = float(np.linalg.norm(e))
        if el > 0 and dl > 0:
            sin2 = min(sin2, float((np.cross(d, e) ** 2).sum()) / (dl * dl * el * el))
    dst_pair = min(16 * EPS * (1 + (far / max(dl, 1e-300)) + (far / max(L, 1e-300))) / max(sin2, 1e-300), 1.0)
    return below, 2 * duv * Lp + dst_pair * (dl + L) + below


def test_the_checker_against_a_float64_twin_by_golden_section(rtx):
    """The key of every (segment, triangle) pair of the batch within the tolerance, and winners — between the two triangles of "two" —
    where the twin's two best are further apart than it.  The batch is chosen for the tolerance, by geometry alone: the tolerance grows
    with (distance / edge)^4, so every segment is drawn NEAR the triangle it is compared with (a well-shaped triangle, P0 within 0.5 edges of its centroid
    on every axis, an axis of about an edge in a random direction).  A pair whose tolerance still exceeds a hundredth of the triangle's longest edge (nearly
    parallel to an edge, a sliver) says nothing and is left out; that share is capped at 2 %."""
    left_out = compared = winners = 0
    rng = np.random.default_rng(31)
    for name, picks, per in (("two", 2, 300), ("plane", 24, 30), ("mixed", 48, 30), ("Knight", 48, 24)):
        s, t, m = buffers_of(rtx, name)
        live = kc._live(m)
        # well-shaped triangles only (longest edge^4 <= 6 |cross|^2): the tolerance's 118 eps L^4 / N2 term is a sliver's
        Af, Bf, Cf = (np.asarray(t[k][live], np.float64) for k in ("posA", "posB", "posC"))
        longest = np.maximum(np.maximum(np.linalg.norm(Bf - Af, axis=1), np.linalg.norm(Cf - Af, axis=1)), np.linalg.norm(Cf - Bf, axis=1))
        live = live[longest ** 4 <= 6 * (np.cross(Bf - Af, Cf - Af) ** 2).sum(1)]
        pick = live[rng.permutation(len(live))[:picks]]
        for j in pick:
            a, b, c = (np.asarray(t[k][j], np.float64) for k in ("posA", "posB", "posC"))
            edge = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
            p0 = (a + b + c) / 3 + rng.uniform(-0.5, 0.5, (per, 3)) * edge
            g = kc.segments_of(rtx, p0, d=rng.standard_normal((per, 3)) * edge * rng.uniform(0.2, 0.8, (per, 1)))
            others = pick if name == "two" else np.array([j])
            keys, _ = kc.oracle_keys(rtx, s[:0], t[others], g)
            T = [tuple(np.asarray(t[k][o], np.float64) for k in ("posA", "posB", "posC")) for o in others]
            for i in range(per):
                q0, d = g["origin"][i].astype(np.float64), g["direction"][i].astype(np.float64)
                want = np.sqrt(np.array([kc.twin_key64(q0, d, *tri)[0] for tri in T]))
                tol = np.array([_tolerance(q0, d, *tri) for tri in T])
                got = np.sqrt(keys[i].astype(np.float64))
                usable = tol[:, 1] <= 0.01 * edge
                left_out += int((~usable).sum())
                compared += int(usable.sum())
                bad = usable & ((got < want - tol[:, 0]) | (got > want + tol[:, 1]))
                assert not bad.any(), (name, int(j), i, got[bad][:3], want[bad][:3], tol[bad][:3])
                if len(T) > 1 and usable.all():
                    o = np.argsort(want)
                    if want[o[1]] - want[o[0]] > tol[o[0], 1] + tol[o[1], 0]:
                        assert int(np.argmin(got)) == int(o[0]), (name, i)
                        winners += 1
            if name == "two":
                break                                   # (both triangles are compared with every segment: one round)
    share = left_out / (left_out + compared)
    print(f"twin: {compared} pairs compared, {left_out} left out ({100 * share:.2f} %), {winners} winners compared")
    assert compared > 3000 and winners > 100 and share <= 0.02


# ---- (d) the mutants ------------------------------------------------------------------------------------------------------------------------
def _mutant_cases(rtx):
    none, tri, two = _scene(rtx)
    ball = spheres_of(rtx, [(0, 0, 0)], [2.0])
    none_t = tri[:0]
    return [(none, tri, (2, 1, -2), (1, 1, 2)),             # pierces, nothing else is at 0: no piercing
            (none, tri, (1, 1, 2), (2, 1, 2)),              # the endpoints tie: <= moves s to 1
            (none, tri, (5, 5, 9), (1, 1, 1)),              # P1 is nearest: no endpoint P1
            (none, tri, (2, -1, 3), (2, -1, -3)),           # beside edge AB
            (none, tri, (-1, 2, 3), (-1, 2, -3)),           # beside edge AC
            (none, tri, (3, 3, 2), (3, 3, -2)),             # beside edge BC
            (none, tri, (5, -3, 0), (5, -1, 0)),            # the pair's s0 lies beyond the segment: unclamped s
            (ball, none_t, (-4, 1, 0), (4, 1, 0))]          # through the ball: shell sphere


@pytest.mark.parametrize("mutant", list(kc.MUTANTS))
def test_every_mutant_differs_on_a_hand_case(rtx, mutant):
    caught = []
    for i, (s, t, p0, p1) in enumerate(_mutant_cases(rtx)):
        a, b = ask(rtx, s, t, p0, p1, k=2, a=1), ask(rtx, s, t, p0, p1, k=2, a=1, variant=kc.MUTANTS[mutant])
        if kc.different(rtx, a, b):
            caught.append(i)
    print(mutant, "differs on hand cases", caught)
    assert caught, mutant


def test_the_origin_bound_takes_both_endpoints(rtx):
    g = kc.segments_of(rtx, [(1, 2, 3), (0, 0, 0), (5, 5, 5), (7e3, 0, 0)], d=[(1e4, 0, 0), (0, -2e4, 0), (9e9, 0, 0), (np.inf, 0, 0)],
                       radius=[1.0, np.inf, 0.0, 1.0])
    assert kc.origin_bound(rtx, g) == 20000.0                   # (tMax = 0 is left out; an infinite P1 is not finite, its P0 counts)
    assert kc.origin_bound(rtx, g, kc.BOUND_FROM_P0) == 7000.0
    assert kc.origin_bound(rtx, g[:1]) == float(np.float32(1) + np.float32(1e4))


# ---- (e) the boundary -----------------------------------------------------------------------------------------------------------------------
def test_capsule_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_capsule" not in k[".name"]:
                continue
            names[k[".name"]] = (k[".vgpr_count"], k[".sgpr_count"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_capsule (VGPRs, SGPRs):", names)
    assert len(names) == 4, sorted(names)           # f16 / f32 nodes x plain / counting


def _recorded_tracer(rtx, fail=None):
    lib = cabi_record.Recorder(rtx._cabi.PARAMS.itemsize, fail=fail)
    t = object.__new__(rtx._cabi.Tracer)
    t._lib, t._ctx = lib, cabi_record.CTX
    return t, lib


def _options(log):
    return [(e["args"][1], e["args"][2]) for e in log if e["call"] == "rt_set_option"]


def test_capsule_py_refuses_bad_input_before_any_c_call_and_restores_the_options(rtx):
    cp = rtx.capsule
    t, lib = _recorded_tracer(rtx)
    a3 = np.zeros((4, 3), np.float32)
    for p0, p1, radius in ((np.zeros((4, 2), np.float32), a3, 1.0), (a3, np.zeros((3, 3), np.float32), 1.0), (np.zeros(4, np.float32), a3, 1.0),
                           (np.zeros((4, 3), "U1"), a3, 1.0), (a3, a3, np.ones(3)), (a3, a3, np.ones((4, 1))), (a3, a3, "x")):
        for fn in (cp.overlap_capsule, cp.check_capsule, cp.closest_to_segment):
            with pytest.raises(ValueError):
                fn(t, p0, p1, radius)
    for k in (0, 9, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            cp.overlap_capsule(t, a3, a3, 1.0, k)
    for fn in (cp.overlap_capsule, cp.check_capsule, cp.closest_to_segment):
        with pytest.raises(TypeError):
            fn(object(), a3, a3, 1.0)
    assert lib.log == []                                            # not one C call so far
    b3 = a3 + np.float32([1, 2, 3])
    r = cp.overlap_capsule(t, a3, b3, [1, 2, 3, 4], 5, count_all=True)
    assert r.shape == (4, 5) and r.dtype == rtx.CLOSEST
    assert [e["call"] for e in lib.log] == ["rt_set_option"] * 3 + ["rt_closest_points"] + ["rt_set_option"] * 3
    assert _options(lib.log) == [("bytes:closest_capsule", 1), ("bytes:closest_k", 5), ("bytes:closest_all", 1),
                                 ("bytes:closest_capsule", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)]
    segs = np.frombuffer(bytes.fromhex(lib.log[3]["args"][1][len("record:"):]), rtx.RAY)
    assert (segs["origin"] == 0).all() and (segs["direction"] == (1, 2, 3)).all() and list(segs["tMax"]) == [1, 2, 3, 4] and lib.log[3]["args"][2] == 4
    assert cp.check_capsule(t, a3, b3, 0.5).shape == (4,) and cp.check_capsule(t, a3, b3, 0.5).dtype == np.uint8
    rec, s = cp.closest_to_segment(t, a3, b3)
    assert rec.shape == (4,) and s.shape == (4,) and s.dtype == np.float32 and t._closest_k == 1
    # a call that fails still puts the defaults back; so does a restoring call that fails
    t, lib = _recorded_tracer(rtx, fail={"rt_closest_points": -2})
    with pytest.raises(rtx.RtError):
        cp.overlap_capsule(t, a3, b3, 1.0, 3)
    assert _options(lib.log)[-3:] == [("bytes:closest_capsule", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)] and t._closest_k == 1
    t, lib = _recorded_tracer(rtx)
    lib.returns["rt_set_option"] = lambda ctx, name, value: -2 if (name, value) == (b"closest_capsule", 0) else 0
    with pytest.raises(rtx.RtError):
        cp.overlap_capsule(t, a3, b3, 1.0, 3)
    assert _options(lib.log)[-3:] == [("bytes:closest_capsule", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)] and t._closest_k == 1
    mt = object.__new__(rtx._cabi.MultiTracer)
    lib = cabi_record.Recorder(rtx._cabi.PARAMS.itemsize)
    mt._lib, mt._m = lib, cabi_record.MULTI
    assert cp.overlap_capsule(mt, a3, b3, 1.0, 2).shape == (4, 2)
    assert [e["call"] for e in lib.log] == ["rt_multi_set_option"] * 3 + ["rt_multi_closest_points"] + ["rt_multi_set_option"] * 3


def test_the_header_documents_the_option_and_declares_nothing_new(rtx):
    text = open(f"{ROOT}/include/rt.h").read()
    options = text[text.index("int rt_set_option") - 16000:text.index("int rt_set_option")]
    assert '"closest_capsule"' in options and "capsule overlap queries" in options
    assert text.index("/* ---- box overlap queries") < text.index("/* ---- capsule overlap queries") < text.index("/* ---- multi-hit ray queries")
    section = text[text.index("/* ---- capsule overlap queries"):text.index("/* ---- multi-hit ray queries")]
    for word in ("P1 = P0 + d", "dd == 0", "den = dd * ee - b * b", "clamp01(-c / dd)", "(1 - t, t)", "1e-6f", "k < R * R", "min(total, K)",
                 "(k, kind, primitive)", "_reserved[1]", "rt_read_bvh_order", '"closest_count"', "rt_multi_closest_points",
                 "rt_closest_points_device", '"closest_box"', "SOLID", "P0 + d over the inputs", "2^-19"):
        assert word in section, word
    design = open(f"{ROOT}/DESIGN.md").read()
    assert "### Capsule overlap queries" in design and "k_capsule" in design and "segment_triangle" in design
    assert '"closest_capsule"' in open(f"{ROOT}/README.md").read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", bare))
    assert declared == set(rtx._cabi.SYMBOLS) and len(declared) == 115
    assert not any("capsule" in s or "segment" in s for s in declared)
    assert os.path.exists(os.path.join(ROOT, "ray-tracing-extended_amd", "capsule.py")) and hasattr(rtx, "capsule")
    cs = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs", "RtCapsule.cs")).read()
    assert "struct" not in cs and "[DllImport" not in cs and "static class RtCapsule" in cs
    native = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs", "RtNative.cs")).read()
    for call in set(re.findall(r"RtNative\.(rt_[a-z_]+)\(", cs)):
        assert re.search(r"\b" + call + r"\s*\(", native), call
