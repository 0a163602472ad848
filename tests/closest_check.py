"""The checker of the closest-point queries: tests/closest_oracle.c bound with ctypes, a float64 numpy restatement of the same
definition written from the text of include/rt.h, and what the closest-point tests share.  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

_lib = None


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("closest_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        so.cp_closest.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp]
        so.cp_closest.restype = ci
        _lib = so
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def points_of(rtx, xyz, radius=np.inf):
    """RAY (n,): the points xyz (n, 3) with the search radius (a scalar or (n,))"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pts = np.zeros(len(xyz), rtx.RAY)
    pts["origin"] = xyz
    pts["tMax"] = radius
    return pts


def oracle_closest(rtx, spheres, tris, infos, points, chunk_mesh=None, count=False, at_best=None):
    """CLOSEST (n,): the brute-force answer for every point (and the candidates it examined, if asked for).  at_best: an int32 (n,) array
    that receives, per point, the candidates at the winner's key (oracle_candidates)"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    cm = None if chunk_mesh is None else np.ascontiguousarray(chunk_mesh, np.int32)
    assert cm is None or len(cm) == len(m)
    out = np.zeros(len(r), rtx.CLOSEST)
    tests = ctypes.c_uint64(0)
    rc = lib().cp_closest(_p(s), len(s), _p(t), len(t), _p(m), len(m), None if cm is None else _p(cm), _p(r), len(r), _p(out),
                          ctypes.cast(ctypes.byref(tests), ctypes.c_void_p), None if at_best is None else _p(at_best))
    assert rc == 0, f"cp_closest failed: {rc}"
    return (out, tests.value) if count else out


def oracle_candidates(rtx, spheres, tris, infos, points, chunk_mesh=None):
    """int32 (n,): per point, how many candidates below R * R have a key bit-equal to the winner's — 0 for a miss, 1 for an untied
    answer, 2 or more where the tie rule (sphere first, then the lower uploaded index) decided: what query_check.oracle_candidates is
    for rays"""
    n = len(np.ascontiguousarray(points, rtx.RAY).reshape(-1))
    at_best = np.zeros(n, np.int32)
    oracle_closest(rtx, spheres, tris, infos, points, chunk_mesh, at_best=at_best)
    return at_best


def assert_same_records(rtx, got, want, what):
    """every field of every record bit for bit (NaN equal to NaN where the bits agree: the records are compared as words)"""
    got, want = np.ascontiguousarray(got, rtx.CLOSEST).reshape(-1), np.ascontiguousarray(want, rtx.CLOSEST).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 16), want.view(np.uint32).reshape(-1, 16)
    gf, wf = got.view(np.float32).reshape(-1, 16), want.view(np.float32).reshape(-1, 16)
    is_float = np.zeros(16, bool)
    is_float[[0, 1, 2, 3, 4, 5, 6, 11, 12]] = True
    same = (g == w) | (is_float[None, :] & np.isnan(gf) & np.isnan(wf))
    if not same.all():
        rows = np.flatnonzero(~same.all(1))
        i = int(rows[0])
        raise AssertionError(f"{what}: {len(rows)} of {len(got)} records differ; first at {i}:\n got  {got[i]!r}\n want {want[i]!r}")


# ---- the float64 twin: include/rt.h's text again, in numpy float64, one point against all primitives ----------------------------------
def twin64(p, R, sphere_c, sphere_r, A, B, C):
    """(keys, kinds, prims, dst): the float64 keys of every candidate of point p — spheres (centres (ns, 3), radii (ns,)) then triangles
    (A, B, C (nt, 3)) — in (k, kind, primitive) order with k < R^2 applied, and the winner's distance; empty arrays for a miss"""
    p = np.asarray(p, np.float64)
    keys, kinds, prims = [], [], []
    if len(sphere_c):
        m = p - np.asarray(sphere_c, np.float64)
        ds = np.abs(np.sqrt((m * m).sum(1)) - np.asarray(sphere_r, np.float64))
        keys.append(ds * ds); kinds.append(np.full(len(ds), 1)); prims.append(np.arange(len(ds)))
    if len(A):
        keys.append(_tri_keys64(p, np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(C, np.float64)))
        kinds.append(np.full(len(A), 2)); prims.append(np.arange(len(A)))
    if not keys:
        return np.zeros(0), np.zeros(0, int), np.zeros(0, int), np.inf
    k, kind, prim = np.concatenate(keys), np.concatenate(kinds), np.concatenate(prims)
    ok = k < np.float64(R) * np.float64(R)
    k, kind, prim = k[ok], kind[ok], prim[ok]
    o = np.lexsort((prim, kind, k))
    k, kind, prim = k[o], kind[o], prim[o]
    return k, kind, prim, (np.sqrt(k[0]) if len(k) else np.inf)


EPS = 2.0 ** -24


def dst_tolerance(p, kind, prim, sphere_c, sphere_r, A, B, C):
    """How far the checker's float32 distance from p to ONE primitive can lie from that primitive's exact distance: (below, above).
    It is tests/test_closest_cpu.py's derivation with nothing fixed: every magnitude in it is measured on the primitive and the point
    given, so it holds 1e5 units from the origin as it does in the unit cube.

    A triangle (kind 2).  L = max(|eAB|, |eAC|, |p - A|), N2 = |cross(eAB, eAC)|^2, M = |p| + L (a bound on every coordinate that is
    formed).  test_closest_cpu.py: |error of u|, |error of v| <= 118 eps L^4 / N2 + eps, and u, v are brought back into [0, 1], so
    neither error exceeds 1; q moves by at most (|du| + |dv|) L, and the distance to a point of the triangle |dq| from the closest one
    is at most |dq| larger.  It cannot be smaller than the minimum by more than the rounding of q, e and k themselves, 8 eps M, whatever
    u and v came out as (a sliver, a zero-area triangle: N2 = 0): q is a point of the triangle up to that rounding.  So
        below = 8 eps M,        above = 2 min(118 eps L^4 / N2 + eps, 1) L + 8 eps M.
    A sphere (kind 1).  m = p - c carries one rounding per component, dot(m, m) three products and two sums, the root one more:
    |error of len| <= (1 + 5 / 2 + 1) eps len; len - radius one more rounding.  below = above = 6 eps (len + radius).

    The checker's answer is a minimum over primitives and so is the twin's: the checker's dst is at most `above` of the twin's winner
    over the twin's dst, and at most `below` of its own winner under it."""
    p = np.asarray(p, np.float64)
    if kind == 1:
        t = 6 * EPS * (np.linalg.norm(p - np.asarray(sphere_c[prim], np.float64)) + float(sphere_r[prim]))
        return t, t
    a, b, c = (np.asarray(x[prim], np.float64) for x in (A, B, C))
    L = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(p - a))
    N2 = float((np.cross(b - a, c - a) ** 2).sum())
    below = 8 * EPS * (np.linalg.norm(p) + L)
    duv = min(118 * EPS * L ** 4 / N2 + EPS, 1.0) if N2 > 0 else 1.0
    return below, 2 * duv * L + below


def _tri_keys64(p, A, B, C):
    """squared distance from p to every triangle, by clamped projection onto the plane and the three edges — a different route to the same
    minimum than the header's region test (the minimum over the interior projection, where it lies inside, and the three segments)"""
    ab, ac, bc = B - A, C - A, C - B

    def seg(P, d):
        dd = (d * d).sum(1)
        t = np.where(dd > 0, ((p - P) * d).sum(1) / np.where(dd > 0, dd, 1.0), 0.0)
        t = np.clip(t, 0.0, 1.0)
        e = p - (P + d * t[:, None])
        return (e * e).sum(1)
    best = np.minimum(np.minimum(seg(A, ab), seg(A, ac)), seg(B, bc))
    n = np.cross(ab, ac)
    nn = (n * n).sum(1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    ap = p - A
    # barycentrics of the projection
    u = (np.cross(ap, ac) * n).sum(1) / nn1
    v = (np.cross(ab, ap) * n).sum(1) / nn1
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
    h = (ap * n).sum(1)
    plane = h * h / nn1
    return np.where(inside, np.minimum(best, plane), best)
