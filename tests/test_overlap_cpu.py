"""Box overlap queries without a GPU: the checker (tests/overlap_oracle.c) pinned independently of the kernel, and the boundary.

(a) The exact twin.  On coordinates that are multiples of 2^-4 every expression of the touch predicates is an integer in units of 2^-4,
2^-8 or 2^-12, and float32 holds it exactly while it stays below 2^24.  With centres, half-extents and vertices in [-4, 4] (|k| <= 64 in
units of 2^-4) a difference is at most D = 128 units, a cross component at most 2 D^2 = 2^15, the plane's d and rr at most 6 D^3 < 2^24,
an edge axis' p and r at most 2 D^2: all exact.  (|x| < 64 alone would not do: 6 D^3 passes 2^24 from D = 141.)  There the checker's
decision must equal exact geometry: the triangle clipped against the closed box in rational arithmetic (Sutherland-Hodgman, the result
not empty), and for a sphere the exact distance from its centre to the box against its radius.  No case is left out.
(b) The float64 twin on random float scenes: the same axes in float64 from the uploaded corners; decisions must agree except where the
twin itself is within 1e-5 (relative to the axis' r / rr, or to the half-extent for the bounds) of changing its mind.
(c) Records, order, counts.  (d) The boundary: the kernels in the code object, overlap.py's refusals and its `finally`, the header."""
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import cabi_record
import closest_check as cc
import overlap_check as oc
from test_camera_batch_cpu import built_library
from test_gpu_closest import NAMES, batch_of, buffers_of
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


# ---- (a) the exact twin -------------------------------------------------------------------------------------------------------------------
def clip_not_empty(tri, lo, hi):
    """the triangle (three integer points) clipped against the closed box [lo, hi], exactly: True when something is left"""
    poly = [tuple(F(int(x)) for x in v) for v in tri]
    for axis in range(3):
        for bound, sign in ((F(int(lo[axis])), 1), (F(int(hi[axis])), -1)):
            inside = lambda v: sign * (v[axis] - bound) >= 0        # noqa: E731
            out = []
            for i, cur in enumerate(poly):
                prev = poly[i - 1]
                if inside(cur) != inside(prev):
                    s = (bound - prev[axis]) / (cur[axis] - prev[axis])
                    out.append(tuple(prev[a] + (cur[a] - prev[a]) * s for a in range(3)))
                if inside(cur):
                    out.append(cur)
            poly = out
            if not poly:
                return False
    return True


def exact_cases(rng, n):
    """integer (units of 2^-4) triangles A, B, C, box centres c and half-extents h, all |k| <= 64: random ones, degenerate ones (a point,
    a segment, collinear corners), axis-aligned and coplanar-with-a-face ones, and boxes that touch a vertex, an edge or the plane exactly"""
    A, B, C = (rng.integers(-64, 65, (n, 3)) for _ in range(3))
    c = rng.integers(-40, 41, (n, 3))
    h = rng.integers(0, 25, (n, 3))
    kind = rng.integers(0, 10, n)
    for i in range(n):
        k = kind[i]
        if k == 0:
            B[i] = A[i]                                             # a segment A C (or a point)
            if rng.random() < 0.3:
                C[i] = A[i]
        elif k == 1:                                                # collinear: C = A + 2 (B - A) where that stays in range
            B[i] = A[i] + rng.integers(-16, 17, 3)
            C[i] = A[i] + 2 * (B[i] - A[i])
        elif k == 2:                                                # the triangle in a plane of a box face
            a = rng.integers(0, 3)
            A[i, a] = B[i, a] = C[i, a] = c[i, a] + h[i, a] * rng.choice([-1, 1])
        elif k == 3:                                                # a face of the box on a vertex
            a = rng.integers(0, 3)
            c[i] = A[i]
            c[i, a] = A[i, a] + h[i, a] * rng.choice([-1, 1])
        elif k == 4:                                                # a box edge or corner on a vertex
            sg = rng.choice([-1, 1], 3)
            sg[rng.integers(0, 3)] *= rng.integers(0, 2)
            c[i] = B[i] + h[i] * sg
        elif k == 5:                                                # the centre on the triangle's plane: a point of it, small box
            c[i] = (A[i] + B[i]) // 2 if rng.random() < 0.5 else (A[i] + C[i]) // 2
            h[i] = rng.integers(0, 4, 3)
        elif k == 6:                                                # a point box on a vertex or anywhere
            h[i] = 0
            if rng.random() < 0.5:
                c[i] = C[i]
        elif k == 7:                                                # a small box near a long thin triangle's bounds: edge axes decide
            h[i] = rng.integers(1, 6, 3)
            mn, mx = np.minimum(np.minimum(A[i], B[i]), C[i]), np.maximum(np.maximum(A[i], B[i]), C[i])
            c[i] = np.where(rng.random(3) < 0.5, mn + h[i], mx - h[i])
    c = np.clip(c, -64, 64)
    for X in (A, B, C):
        np.clip(X, -64, 64, out=X)
    return A, B, C, c, h


def test_exact_twin_triangles(rtx):
    rng = np.random.default_rng(20271)
    n = 4000
    A, B, C, c, h = exact_cases(rng, n)
    u = np.float32(1 / 16)
    t = tris_of(rtx, A * u, B * u, C * u)
    boxes = oc.boxes_of(rtx, c * u, h * u)
    none = np.zeros(0, rtx.SPHERE)
    touched = degenerate = counted_out = 0
    for i in range(n):
        got = int(oc.oracle_touches(rtx, none, t[i:i + 1], boxes[i:i + 1])[0, 0])
        want = clip_not_empty((A[i], B[i], C[i]), c[i] - h[i], c[i] + h[i])
        assert got == int(want), (i, A[i], B[i], C[i], c[i], h[i], got, want)
        touched += got
        # counts: a touching candidate counts unless its key is NaN (closest_oracle's record for c is then the miss record)
        total = int(oc.counts(oc.oracle_overlap(rtx, none, t[i:i + 1], one_chunk(rtx, 1), boxes[i:i + 1], 1, 1))[0, 0])
        keyed = int(cc.oracle_closest(rtx, none, t[i:i + 1], one_chunk(rtx, 1), cc.points_of(rtx, [c[i] * u]))["kind"][0] != 0)
        assert total == (got & keyed), (i, total, got, keyed)
        if not np.cross(B[i] - A[i], C[i] - A[i]).any():
            degenerate += 1
            counted_out += got & (1 - keyed)
    print(f"exact twin: {n} triangles, {touched} touch, {degenerate} degenerate, {counted_out} touching with a NaN key")
    assert n // 5 < touched < 4 * n // 5 and degenerate > n // 10


def test_exact_twin_spheres(rtx):
    rng = np.random.default_rng(20272)
    n = 2000
    sc, r = rng.integers(-64, 65, (n, 3)), rng.integers(0, 40, n)
    c, h = rng.integers(-40, 41, (n, 3)), rng.integers(0, 25, (n, 3))
    for i in range(0, n, 4):                                        # tangent on purpose: the ball's extreme point on a face
        a = rng.integers(0, 3)
        sc[i] = c[i]
        sc[i, a] = c[i, a] + (h[i, a] + r[i]) * rng.choice([-1, 1])
    sc = np.clip(sc, -128, 128)
    u = np.float32(1 / 16)
    got = oc.oracle_touches(rtx, spheres_of(rtx, sc * u, r * u), np.zeros(0, rtx.TRIANGLE), oc.boxes_of(rtx, c * u, h * u))
    e = np.maximum(np.maximum((c - h) - sc, sc - (c + h)), 0)
    want = (e * e).sum(1) <= r * r                                  # (integers: exact)
    assert np.array_equal(got[np.arange(n), np.arange(n)], want.astype(np.uint8))
    tangent = ((e * e).sum(1) == r * r).sum()
    print(f"exact twin: {n} spheres, {int(want.sum())} touch, {int(tangent)} tangent")
    assert tangent >= n // 8 and n // 5 < want.sum() < 4 * n // 5


# ---- (b) the float64 twin -------------------------------------------------------------------------------------------------------------------
def twin64(A, B, C, c, h):
    """float64 from the uploaded corners: (the smallest slack over the 16 conditions, each relative to its own scale).  slack > 0: the
    intervals overlap on that axis; the twin's decision is `all slacks >= 0`"""
    A, B, C, c, h = (np.asarray(x, np.float64) for x in (A, B, C, c, h))
    rel = []
    mn, mx = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
    for a in range(3):
        scale = max(h[a], 1e-300)
        rel += [((c[a] + h[a]) - mn[a]) / scale, (mx[a] - (c[a] - h[a])) / scale]
    v = [A - c, B - c, C - c]
    e0, e2 = B - A, C - A
    n = np.cross(e0, e2)
    rr = (h * np.abs(n)).sum()
    rel.append((rr - abs(n @ v[0])) / max(rr, 1e-300))
    for f in (e0, e2 - e0, e2):
        for a in range(3):
            ax = np.cross(np.eye(3)[a], f)
            p = [ax @ vj for vj in v]
            r = (h * np.abs(ax)).sum()
            rel += [(r - min(p)) / max(r, 1e-300), (max(p) + r) / max(r, 1e-300)]
    return min(rel)


def test_checker_against_the_float64_twin(rtx):
    """random triangles of edge ~0.4 in the unit cube, boxes of half-extents 0.05 .. 0.35 (comparable to the triangles: with much smaller
    boxes float32's error, which is relative to the coordinates, grows against r)"""
    rng = np.random.default_rng(20273)
    n = 6000
    A = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    B = (A + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    C = (A + rng.uniform(-0.4, 0.4, (n, 3))).astype(np.float32)
    c = (A + rng.uniform(-0.5, 0.5, (n, 3))).astype(np.float32)
    h = rng.uniform(0.05, 0.35, (n, 3)).astype(np.float32)
    t = tris_of(rtx, A, B, C)
    boxes = oc.boxes_of(rtx, c, h)
    got = oc.oracle_touches(rtx, np.zeros(0, rtx.SPHERE), t, boxes)[np.arange(n), np.arange(n)]
    left_out = yes = 0
    for i in range(n):
        slack = twin64(A[i], B[i], C[i], c[i], h[i])
        if abs(slack) < 1e-5:
            left_out += 1
            continue
        assert int(got[i]) == int(slack > 0), (i, slack, got[i])
        yes += int(slack > 0)
    print(f"float64 twin: {n} cases, {yes} touch, {left_out} left out ({100.0 * left_out / n:.3f} %)")
    assert left_out <= n // 50 and n // 5 < yes < 4 * n // 5


# ---- (c) records, order, counts ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(rtx):
    cache = {}

    def get(name):
        if name not in cache:
            s, t, m = buffers_of(rtx, name)
            p = oc.batch_of(rtx, s, t, m, batch_of(rtx, s, t, m))
            p.setflags(write=False)
            cache[name] = (s, t, m, p)
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_counts_prefixes_and_order(rtx, batches, name):
    s, t, m, p = batches(name)
    totals = np.zeros(len(p), np.int32)
    full = oc.oracle_overlap(rtx, s, t, m, p, 8, 0, totals=totals)
    for k in range(1, 9):
        for count_all in (0, 1):
            r = oc.oracle_overlap(rtx, s, t, m, p, k, count_all)
            want = totals if count_all else np.minimum(totals, k)
            assert np.array_equal(oc.counts(r), np.repeat(want[:, None], k, 1)) and (r["_reserved"][..., 1] == 0).all(), (name, k, count_all)
            a, b = oc.words(rtx, r).copy(), oc.words(rtx, full[:, :k]).copy()
            a[..., oc.COUNT_WORD] = b[..., oc.COUNT_WORD] = 0
            assert np.array_equal(a, b), (name, k, count_all)
            assert ((r["kind"] != 0).sum(1) == np.minimum(totals, k)).all()
    d = full["dst"]
    with np.errstate(invalid="ignore"):
        assert (np.diff(d, axis=1)[np.isfinite(d[:, 1:])] >= 0).all()
    # the totals are the touch decisions' (every triangle of these scenes is addressed by a chunk and has a key)
    touch = oc.oracle_touches(rtx, s, t, p)
    whole = len(p) - 9                                              # batch_of: the box over the whole scene, then nothing, then seven unsearched
    near = np.r_[0:whole - 2, whole:len(p)]                         # (all but the two far boxes, where a key can overflow to inf - inf = NaN)
    assert np.array_equal(touch.sum(1)[near], totals[near])
    assert totals[whole] == len(s) + len(t) and (totals[whole + 1:] == 0).all() and (full["kind"][whole + 1:] == 0).all()
    # the two far boxes in front of it: everything touches, every key is +inf, and the order is (kind, uploaded index) alone
    # (a triangle whose region test overflows to inf - inf has a NaN key and does not count: a few of Knight's)
    for far in (whole - 2, whole - 1):
        assert touch[far].all() and 0.9 * (len(s) + len(t)) <= totals[far] <= len(s) + len(t)
        listed = full[far][:min(8, totals[far])]
        assert np.isposinf(listed["dst"]).all() and (listed["kind"] != 0).all()
        ids = list(zip(listed["kind"].tolist(), listed["primitive"].tolist()))
        assert ids == sorted(ids) and len(set(ids)) == len(ids), (name, far, ids)


@pytest.mark.parametrize("name", ["mixed", "plane", "spheres"])
def test_record_0_is_the_closest_point_among_the_touching(rtx, batches, name):
    """per box: the scene with every candidate that does not touch made unable to win (NaN corners, a NaN radius — indices and chunks
    stay), asked for the closest point of c by closest_oracle.c: record 0 at K = 1 in every word but the count"""
    s, t, m, p = batches(name)
    touch = oc.oracle_touches(rtx, s, t, p)
    got = oc.oracle_overlap(rtx, s, t, m, p, 1, 0)[:, 0]
    rng = np.random.default_rng(5)
    touching = np.flatnonzero(touch.sum(1) > 0)
    some = np.unique(np.r_[rng.integers(0, len(p), 40), rng.permutation(touching)[:60], np.flatnonzero(touch.sum(1) > 1)[:40]])
    some = some[(some != len(p) - 11) & (some != len(p) - 10)]      # (not the two far boxes: closest_oracle.c's k < R * R never takes a key of +inf)
    hits = 0
    for i in some:
        s2, t2 = s.copy(), t.copy()
        s2["radius"][touch[i, :len(s)] == 0] = np.nan
        t2["posA"][touch[i, len(s):] == 0] = np.nan
        want = cc.oracle_closest(rtx, s2, t2, m, cc.points_of(rtx, [p["origin"][i]]))[0]
        g = oc.words(rtx, got[i:i + 1]).copy()
        assert g[0, oc.COUNT_WORD] == (1 if touch[i].any() else 0)
        g[0, oc.COUNT_WORD] = 0
        cc.assert_same_records(rtx, g.view(rtx.CLOSEST).reshape(-1), np.array([want]), f"{name} box {i}")
        hits += int(touch[i].any())
    assert hits > 20


def test_the_batches_hold_what_they_promise(rtx, batches):
    """boxes that only the edge axes reject, boxes that only the plane rejects, ties at the K-th key, touching at equal coordinates"""
    for name in ("plane", "mixed", "Knight", "Suzanne"):
        s, t, m, p = batches(name)
        totals = {v: np.zeros(len(p), np.int32) for v in (oc.DEFINITION, oc.BOUNDS_ONLY, oc.NO_PLANE, oc.NO_EDGES, oc.OPEN_SETS)}
        ties = np.zeros(len(p), np.int32)
        for v, a in totals.items():
            oc.oracle_overlap(rtx, s, t, m, p, 2, 0, variant=v, totals=a, kth_ties=ties if v == oc.DEFINITION else None)
        differ = {v: int((a != totals[oc.DEFINITION]).sum()) for v, a in totals.items()}
        print(name, len(p), "boxes;", differ, "ties at K = 2:", int(ties.sum()))
        assert differ[oc.BOUNDS_ONLY] >= 10 and differ[oc.NO_EDGES] >= 10 and differ[oc.OPEN_SETS] >= 10 and ties.sum() >= 10, (name, differ)
        assert name == "plane" or differ[oc.NO_PLANE] >= 10, (name, differ)


def test_hand_cases(rtx):
    """one triangle (0,0,0) (4,0,0) (0,4,0) and a unit ball at (0,0,8)"""
    t = tris_of(rtx, [(0, 0, 0)], [(4, 0, 0)], [(0, 4, 0)])
    s = spheres_of(rtx, [(0, 0, 8)], [1.0])
    m = one_chunk(rtx, 1)
    ask = lambda c, h, k=2, a=1, gate=1.0: oc.oracle_overlap(rtx, s, t, m, oc.boxes_of(rtx, [c], h, gate), k, a)[0]    # noqa: E731
    r = ask((1, 1, 0), 0.5)
    assert list(r["kind"]) == [2, 0] and r["dst"][0] == 0 and (oc.counts(r) == 1).all() and tuple(r["point"][0]) == (1, 1, 0)
    # beyond the hypotenuse, inside the bounds: the edge axis BC x z separates.  The corner (3, 3) is sqrt 2 from it; the box reaches 0.5
    assert (ask((3.5, 3.5, 0), 0.5)["kind"] == 0).all()
    # the corner (2, 2, 0) of the box ON the hypotenuse: touching counts
    r = ask((2.5, 2.5, 0), 0.5)
    assert r["kind"][0] == 2 and r["dst"][0] == np.sqrt(np.float32(0.5))
    # above the plane, bounds overlap in x and y: the box's lower face at z = 0 touches, at z = 2^-10 the bounds condition rejects it
    assert ask((1, 1, 0.5), 0.5)["kind"][0] == 2 and (ask((1, 1, 0.5 + 2.0 ** -10), 0.5)["kind"] == 0).all()
    # a point box on the surface and off it
    assert ask((1, 1, 0), 0.0)["kind"][0] == 2 and (ask((1, 1, 0.25), 0.0)["kind"] == 0).all()
    # the solid ball: a box inside it touches (key: the distance from c to the SURFACE, 0.5^2), one tangent at its top does, one above not
    r = ask((0, 0, 8.5), 0.125)
    assert list(r["kind"]) == [1, 0] and r["dst"][0] == 0.5 and r["side"][0] == -1
    assert ask((0, 0, 9.5), 0.5)["kind"][0] == 1 and (ask((0, 0, 9.5 + 2.0 ** -10), 0.5)["kind"] == 0).all()
    # both, nearest to the centre first; sphere before triangle at equal keys (centre (0, 0, 3.5): 3.5 to each)
    r = ask((0, 0, 3.5), 4.0)
    assert list(r["kind"]) == [1, 2] and (r["dst"] == 3.5).all() and (oc.counts(r) == 2).all()
    assert list(ask((0, 0, 3.25), 4.0)["kind"]) == [2, 1]
    # not searched
    for c, h, gate in (((1, 1, 0), 0.5, 0.0), ((1, 1, 0), 0.5, -1.0), ((1, 1, 0), 0.5, np.nan), ((1, 1, 0), -0.5, 1.0), ((1, 1, 0), np.nan, 1.0),
                       ((1, 1, 0), np.inf, 1.0), ((np.nan, 1, 0), 0.5, 1.0), ((1, np.inf, 0), 0.5, 1.0)):
        r = ask(c, h, 3, 1, gate)
        assert (r["kind"] == 0).all() and (r["_reserved"] == 0).all() and np.isposinf(r["dst"]).all() and (r["primitive"] == -1).all()
    # a triangle with a corner at 1e30 or beyond is no candidate, whatever the box
    far = tris_of(rtx, [(0, 0, 0)], [(1e30, 0, 0)], [(0, 4, 0)])
    assert (oc.oracle_overlap(rtx, s[:0], far, m, oc.boxes_of(rtx, [(1, 1, 0)], 0.5), 1, 1)["kind"] == 0).all()


def _hand_cases(rtx):
    """(spheres, triangles, centre, half-extents, K, all) that between them tell every mutant of the checker from the definition"""
    tri = tris_of(rtx, [(0, 0, 0)], [(4, 0, 0)], [(0, 4, 0)])
    ball = spheres_of(rtx, [(0, 0, 8)], [1.0])
    none_s, none_t = ball[:0], tri[:0]
    segment = tris_of(rtx, [(0, 0, 0)], [(0, 0, 0)], [(4, 0, 0)])      # A == B: beside its middle the edge-AB region gives u = 0 / 0
    return [(none_s, tri, (3.5, 3.5, 0), 0.5, 1, 1),                    # inside the bounds, beyond the hypotenuse: an edge axis alone
            (none_s, tris_of(rtx, [(0, 0, 0)], [(4, 0, 2)], [(0, 4, 2)]), (1, 1, 2), 0.25, 1, 1),   # above the interior of the plane
                                                                        # z = (x + y) / 2, inside its bounds and all three projections: the plane alone
            (none_s, tri, (1, 1, 0.5), 0.5, 1, 1),                      # the lower face ON the plane: closed sets
            (ball, none_t, (0, 0, 9.5), 0.5, 1, 1),                     # tangent to the ball
            (none_s, segment, (2, 1, 0), 1.5, 1, 1)]                    # touches, and its key is NaN: it does not count


def test_a_key_of_plus_infinity_counts_and_a_nan_key_does_not(rtx):
    tri = tris_of(rtx, [(0, 0, 0), (0, 0, 1)], [(4, 0, 0), (4, 0, 1)], [(0, 4, 0), (0, 4, 1)])
    ball = spheres_of(rtx, [(0, 0, 8)], [1.0])
    r = oc.oracle_overlap(rtx, ball, tri, one_chunk(rtx, 2), oc.boxes_of(rtx, [(3e19, 0, 0)], 4e19), 4, 0)[0]
    assert list(r["kind"]) == [1, 2, 2, 0] and list(r["primitive"]) == [0, 0, 1, -1] and np.isposinf(r["dst"]).all() and (oc.counts(r) == 3).all()
    r = oc.oracle_overlap(rtx, ball, tri, one_chunk(rtx, 2), oc.boxes_of(rtx, [(3e19, 0, 0)], 4e19), 2, 1)[0]
    assert list(r["kind"]) == [1, 2] and list(r["primitive"]) == [0, 0] and (oc.counts(r) == 3).all()
    s, t, c, h, k, a = _hand_cases(rtx)[-1]
    assert oc.oracle_touches(rtx, s, t, oc.boxes_of(rtx, [c], h))[0, 0] == 1
    r = oc.oracle_overlap(rtx, s, t, one_chunk(rtx, 1), oc.boxes_of(rtx, [c], h), k, a)[0]
    assert (r["kind"] == 0).all() and (oc.counts(r) == 0).all()


@pytest.mark.parametrize("mutant", list(oc.MUTANTS))
def test_every_mutant_differs_on_a_hand_case(rtx, mutant):
    def ask(case, variant):
        s, t, c, h, k, a = case
        return oc.oracle_overlap(rtx, s, t, one_chunk(rtx, len(t)), oc.boxes_of(rtx, [c], h), k, a, variant=variant)
    caught = [i for i, case in enumerate(_hand_cases(rtx)) if oc.different(rtx, ask(case, oc.DEFINITION), ask(case, oc.MUTANTS[mutant]))]
    print(mutant, "differs on hand cases", caught)
    assert caught, mutant


def test_exact_bounds_and_edge_axes_on_the_wider_range(rtx):
    """The issue's range, multiples of 2^-4 with |x| < 64 (|k| < 1024): the plane's d and rr pass 2^24 there, the bounds and the nine edge
    axes do not (a difference <= 2048 units, p and r <= 2 * 2048 * 2048 = 2^23).  So on that range the checker WITHOUT the plane axis
    (variant NO_PLANE) must equal the same fifteen conditions evaluated in Python integers."""
    rng = np.random.default_rng(20274)
    n = 3000
    A, B, C = (rng.integers(-1023, 1024, (n, 3)) for _ in range(3))
    near = rng.random(n) < 0.5
    B[near] = A[near] + rng.integers(-200, 201, (int(near.sum()), 3))
    C[near] = A[near] + rng.integers(-200, 201, (int(near.sum()), 3))
    np.clip(B, -1023, 1023, out=B)
    np.clip(C, -1023, 1023, out=C)
    c = np.clip(A + rng.integers(-300, 301, (n, 3)), -1023, 1023)
    h = rng.integers(0, 200, (n, 3))
    on = rng.random(n) < 0.2                                        # a face of the box on A's coordinate
    c[on, 0] = np.clip(A[on, 0] - h[on, 0], -1023, 1023)
    u = np.float32(1 / 16)
    got = oc.oracle_touches(rtx, np.zeros(0, rtx.SPHERE), tris_of(rtx, A * u, B * u, C * u), oc.boxes_of(rtx, c * u, h * u), variant=oc.NO_PLANE)
    yes = 0
    for i in range(n):
        a, b, cc_, ce, he = (tuple(int(x) for x in v) for v in (A[i], B[i], C[i], c[i], h[i]))
        ok = all(min(a[k], b[k], cc_[k]) <= ce[k] + he[k] and max(a[k], b[k], cc_[k]) >= ce[k] - he[k] for k in range(3))
        v = [tuple(p[k] - ce[k] for k in range(3)) for p in (a, b, cc_)]
        e0, e2 = tuple(b[k] - a[k] for k in range(3)), tuple(cc_[k] - a[k] for k in range(3))
        for f in (e0, tuple(e2[k] - e0[k] for k in range(3)), e2):
            for p, r in (([w[2] * f[1] - w[1] * f[2] for w in v], he[1] * abs(f[2]) + he[2] * abs(f[1])),
                         ([w[0] * f[2] - w[2] * f[0] for w in v], he[0] * abs(f[2]) + he[2] * abs(f[0])),
                         ([w[1] * f[0] - w[0] * f[1] for w in v], he[0] * abs(f[1]) + he[1] * abs(f[0]))):
                ok = ok and min(p) <= r and max(p) >= -r
        assert int(got[i, i]) == int(ok), (i, a, b, cc_, ce, he)
        yes += int(ok)
    print(f"wider range: {n} cases, {yes} pass the bounds and the edge axes")
    assert n // 10 < yes < 9 * n // 10


# ---- (d) the boundary -----------------------------------------------------------------------------------------------------------------------
def test_overlap_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_overlap" not in k[".name"]:
                continue
            names[k[".name"]] = (k[".vgpr_count"], k[".sgpr_count"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_overlap (VGPRs, SGPRs):", names)
    assert len(names) == 4, sorted(names)           # f16 / f32 nodes x plain / counting


def _recorded_tracer(rtx, fail=None):
    lib = cabi_record.Recorder(rtx._cabi.PARAMS.itemsize, fail=fail)
    t = object.__new__(rtx._cabi.Tracer)
    t._lib, t._ctx = lib, cabi_record.CTX
    return t, lib


def _options(log):
    return [(e["args"][1], e["args"][2]) for e in log if e["call"] == "rt_set_option"]


def test_overlap_py_refuses_bad_input_before_any_c_call_and_restores_the_options(rtx):
    ov = rtx.overlap
    t, lib = _recorded_tracer(rtx)
    c3 = np.zeros((4, 3), np.float32)
    for centres, half in ((np.zeros((4, 2), np.float32), 1.0), (np.zeros(4, np.float32), 1.0), (np.zeros((4, 3), "U1"), 1.0),
                          (c3, np.ones(2)), (c3, np.ones((3, 3))), (c3, np.ones((4, 3, 1))), (c3, "x")):
        for fn in (ov.overlap_box, ov.check_box):
            with pytest.raises(ValueError):
                fn(t, centres, half)
    for k in (0, 9, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            ov.overlap_box(t, c3, 1.0, k)
    for lo, hi, shape in (((0, 0), (1, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, -1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 2)),
                          ((0, 0, 0), (1, 1, 1), (2, 0, 2)), ((0, 0, 0), (np.inf, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2.5, 2, 2))):
        with pytest.raises(ValueError):
            ov.voxel_counts(t, lo, hi, shape)
    for fn, args in ((ov.overlap_box, (c3, 1.0)), (ov.check_box, (c3, 1.0)), (ov.voxel_counts, ((0, 0, 0), (1, 1, 1), (2, 2, 2)))):
        with pytest.raises(TypeError):
            fn(object(), *args)
    assert lib.log == []                                            # not one C call so far
    # good input: the three options, the call, the defaults again
    r = ov.overlap_box(t, c3, (1, 2, 3), 5, count_all=True)
    assert r.shape == (4, 5) and r.dtype == rtx.CLOSEST
    assert [e["call"] for e in lib.log] == ["rt_set_option"] * 3 + ["rt_closest_points"] + ["rt_set_option"] * 3
    assert _options(lib.log) == [("bytes:closest_box", 1), ("bytes:closest_k", 5), ("bytes:closest_all", 1),
                                 ("bytes:closest_box", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)]
    boxes = np.frombuffer(bytes.fromhex(lib.log[3]["args"][1][len("record:"):]), rtx.RAY)
    assert (boxes["origin"] == 0).all() and (boxes["direction"] == (1, 2, 3)).all() and (boxes["tMax"] == 1).all() and lib.log[3]["args"][2] == 4
    assert ov.check_box(t, c3, 0.5).shape == (4,) and ov.check_box(t, c3, 0.5).dtype == np.uint8
    assert t._closest_k == 1
    # voxel_counts: one call for a small grid, K = 1 with all, cell-centre boxes
    del lib.log[:]
    v = ov.voxel_counts(t, (0, 0, 0), (4, 2, 1), (4, 2, 1))
    assert v.shape == (4, 2, 1) and v.dtype == np.int32
    assert _options(lib.log)[:3] == [("bytes:closest_box", 1), ("bytes:closest_k", 1), ("bytes:closest_all", 1)]
    call = [e for e in lib.log if e["call"] == "rt_closest_points"]
    assert len(call) == 1 and call[0]["args"][2] == 8
    boxes = np.frombuffer(bytes.fromhex(call[0]["args"][1][len("record:"):]), rtx.RAY)
    assert (boxes["direction"] == 0.5).all() and tuple(boxes["origin"][0]) == (0.5, 0.5, 0.5) and tuple(boxes["origin"][-1]) == (3.5, 1.5, 0.5)
    # a call that fails still puts the defaults back
    t, lib = _recorded_tracer(rtx, fail={"rt_closest_points": -2})
    with pytest.raises(rtx.RtError):
        ov.overlap_box(t, c3, 1.0, 3)
    assert _options(lib.log)[-3:] == [("bytes:closest_box", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)] and t._closest_k == 1
    # a restoring call that fails does not keep the other two from being made
    t, lib = _recorded_tracer(rtx)
    lib.returns["rt_set_option"] = lambda ctx, name, value: -2 if (name, value) == (b"closest_box", 0) else 0
    with pytest.raises(rtx.RtError):
        ov.overlap_box(t, c3, 1.0, 3)
    assert _options(lib.log)[-3:] == [("bytes:closest_box", 0), ("bytes:closest_k", 1), ("bytes:closest_all", 0)] and t._closest_k == 1
    # a MultiTracer takes the same path
    mt = object.__new__(rtx._cabi.MultiTracer)
    lib = cabi_record.Recorder(rtx._cabi.PARAMS.itemsize)
    mt._lib, mt._m = lib, cabi_record.MULTI
    assert ov.overlap_box(mt, c3, 1.0, 2).shape == (4, 2)
    assert [e["call"] for e in lib.log] == ["rt_multi_set_option"] * 3 + ["rt_multi_closest_points"] + ["rt_multi_set_option"] * 3


def test_the_header_documents_the_option_and_declares_nothing_new(rtx):
    text = open(f"{ROOT}/include/rt.h").read()
    options = text[text.index("int rt_set_option") - 16000:text.index("int rt_set_option")]
    assert '"closest_box"' in options and "box overlap queries" in options
    section = text[text.index("/* ---- box overlap queries"):text.index("/* ---- multi-hit ray queries")]
    assert text.index("/* ---- K-nearest queries") < text.index("/* ---- box overlap queries")
    for word in ("half-extents", "tMax > 0", "1e30f", "fabsf(d) <= rr", "f1 = eAC - eAB", "d2 <= R * R", "min(total, K)", "(k, kind, primitive)",
                 "rt_read_bvh_order", '"closest_count"', "rt_multi_closest_points", "rt_closest_points_device", "disjoint", "0.99"):
        assert word in section, word
    design = open(f"{ROOT}/DESIGN.md").read()
    assert "### Box overlap queries" in design and "k_overlap" in design and "box_touches_triangle" in design
    assert '"closest_box"' in open(f"{ROOT}/README.md").read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(rt_[a-z_]+)\s*\(", bare))
    assert declared == set(rtx._cabi.SYMBOLS) and len(declared) == 115
    assert not any("overlap" in s or "box" in s for s in declared)
    assert os.path.exists(os.path.join(ROOT, "ray-tracing-extended_amd", "overlap.py")) and hasattr(rtx, "overlap")
    cs = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs", "RtOverlap.cs")).read()
    assert "struct" not in cs and "[DllImport" not in cs and "static class RtOverlap" in cs
    assert all(f'"{o}"' in cs for o in ("closest_box", "closest_k", "closest_all"))
