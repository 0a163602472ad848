"""The checker of the capsule overlap queries: tests/capsule_oracle.c bound with ctypes, and what the capsule tests share — the batch of
segments every scene gets (module-level `batch_of`), the float64 twin by golden section.  The binding's one call, the word-for-word
comparison, the counts and the scene's bounds are listed_check.py's, shared with nearest_check.py and overlap_check.py.  Test
infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker
from listed_check import (COUNT_WORD, _live, _p, assert_same_records, bind_listed, counts, different, oracle_listed,   # noqa: F401
                          scene_bounds, words)

_lib = None

# capsule_oracle.c's `variant`: the definition and its one-line mutants
DEFINITION, NON_STRICT_REPLACE, UNCLAMPED_S, SHELL_SPHERE, BOUND_FROM_P0 = range(5)
DROP = {"endpoint P1": 12, "edge AB": 13, "edge AC": 14, "edge BC": 15, "piercing": 16}
MUTANTS = {"<= in the replacement rule": NON_STRICT_REPLACE, "unclamped s": UNCLAMPED_S, "shell sphere": SHELL_SPHERE,
           **{"no " + k: v for k, v in DROP.items()}}
FORMS = ((1, 0), (2, 0), (8, 0), (3, 1), (1, 1))    # (K, all) of the GPU tests
S_WORD = 15                                          # _reserved[1] among a record's 16 words: the bits of s


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("capsule_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        bind_listed(so.cp_capsule)
        so.cp_keys.argtypes = [vp, ci, vp, ci, vp, ci, ci, vp, vp]
        so.cp_keys.restype = ci
        so.cp_origin_bound.argtypes = [vp, ci, ci]
        so.cp_origin_bound.restype = ctypes.c_float
        _lib = so
    return _lib


def segments_of(rtx, p0, p1=None, radius=np.inf, d=None):
    """RAY (n,): origin = p0 (n, 3), direction = d, or p1 - p0 formed in float32, tMax = the reach (a scalar or (n,))"""
    p0 = np.asarray(p0, np.float32).reshape(-1, 3)
    g = np.zeros(len(p0), rtx.RAY)
    g["origin"] = p0
    g["direction"] = np.asarray(d, np.float32).reshape(-1, 3) if d is not None else np.asarray(p1, np.float32).reshape(-1, 3) - p0
    g["tMax"] = radius
    return g


def oracle_capsule(rtx, spheres, tris, infos, segs, k, count_all=0, chunk_mesh=None, variant=DEFINITION, totals=None, kth_ties=None):
    """CLOSEST (n, k): the brute-force answer for every segment.  totals / kth_ties as nearest_check.oracle_nearest's"""
    return oracle_listed(lib().cp_capsule, rtx, spheres, tris, infos, segs, k, count_all, chunk_mesh, variant, totals, kth_ties)


def oracle_keys(rtx, spheres, tris, segs, variant=DEFINITION):
    """(keys, s) float32 (n, ns + nt): the checker's key and segment parameter of every segment against every sphere, then every triangle
    in uploaded order"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    r = np.ascontiguousarray(segs, rtx.RAY).reshape(-1)
    keys = np.zeros((len(r), len(s) + len(t)), np.float32)
    par = np.zeros_like(keys)
    assert lib().cp_keys(_p(s), len(s), _p(t), len(t), _p(r), len(r), int(variant), _p(keys), _p(par)) == 0
    return keys, par


def origin_bound(rtx, segs, variant=DEFINITION):
    r = np.ascontiguousarray(segs, rtx.RAY).reshape(-1)
    return float(lib().cp_origin_bound(_p(r), len(r), int(variant)))


def searched(segs):
    """bool (n,): the header's rule — R > 0 (not NaN) and every component of P0, d and P1 = P0 + d (as floats) finite"""
    with np.errstate(over="ignore", invalid="ignore"):
        p1 = segs["origin"] + segs["direction"]
        return (segs["tMax"] > 0) & np.isfinite(segs["origin"]).all(1) & np.isfinite(segs["direction"]).all(1) & np.isfinite(p1).all(1)


def params(records):
    """the float s of every record, from _reserved[1]"""
    return np.array(records["_reserved"][..., 1], np.int32).view(np.float32)


# ---- the batch ------------------------------------------------------------------------------------------------------------------------------
def batch_of(rtx, s, t, m, base, seed=23, per_kind=16):
    """the scene's own closest-point batch `base` (test_gpu_closest.batch_of) read as segments, and per kind up to `per_kind` segments built on
    triangles picked at random:
      * the base points with a random d of a triangle's size, every other searched one with a finite reach; a quarter of them axis-aligned
        (one or two components of d are 0), some along (1, 1, 1), some of length 0, some 10^3 times longer than the scene;
      * through a triangle's centroid along its normal (pierces), starting on it, ending on it, and stopping short of it;
      * parallel to a triangle above its centroid (the endpoints tie), beside an edge with both endpoints far, over a vertex;
      * along an edge, and an edge itself as the segment (d parallel to the edge: the pair's denominator cancels);
      * through, inside and beside the spheres;
      * one segment across the whole scene with R = +inf, and a tiny reach;
      * inputs that are not searched: tMax 0, negative, NaN; a NaN and an infinite endpoint or axis."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(s, t, m)
    ext = np.maximum(hi - lo, 1e-3)
    diag = float(np.linalg.norm(ext))
    live = _live(m)
    out = []
    p = np.ascontiguousarray(base, rtx.RAY).copy()
    if len(live):
        A, B, C = (np.asarray(t[k][live], np.float64) for k in ("posA", "posB", "posC"))
        size = float(np.median(np.maximum(np.abs(B - A), np.abs(C - A)).max(1)))
    else:
        size = float(np.median(s["radius"]))
    n = len(p)
    d = rng.standard_normal((n, 3)) * size
    kind = rng.integers(0, 16, n)
    d[kind == 0, 0] = 0
    d[kind == 1, 1:] = 0
    d[kind == 2] = np.abs(d[kind == 2, :1])                     # along (1, 1, 1)
    d[kind == 3] = 0                                            # a point
    d[kind == 4] *= 1e3 * diag / size                           # far longer than the scene
    d[kind == 5] *= 1e-6                                        # tiny
    p["direction"] = d.astype(np.float32)
    ok = np.flatnonzero(np.isfinite(p["origin"]).all(1) & (p["tMax"] > 0))
    p["tMax"][ok[::2]] = np.float32(diag / 6)
    out.append(p)
    if len(live):
        pick = live[rng.permutation(len(live))[:per_kind]]
        A, B, C = (np.asarray(t[k][pick], np.float64) for k in ("posA", "posB", "posC"))
        cen = (A + B + C) / 3
        nrm = np.cross(B - A, C - A)
        nn = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        edge = np.maximum(np.linalg.norm(B - A, axis=1, keepdims=True), 1e-6)
        R = (2 * edge[:, 0]).astype(np.float32)
        up = nn * edge * 0.5
        out.append(segments_of(rtx, cen + up, cen - up, R))                                          # pierces
        out.append(segments_of(rtx, cen, cen + up, R))                                               # starts on it
        out.append(segments_of(rtx, cen + up, cen, R))                                               # ends on it
        out.append(segments_of(rtx, cen + up, cen + up * 0.25, R))                                   # stops short
        along = (B - A) * 0.25
        out.append(segments_of(rtx, cen + up - along, cen + up + along, R))                          # parallel above the centroid
        outward = np.cross(B - A, nn)
        outward /= np.maximum(np.linalg.norm(outward, axis=1, keepdims=True), 1e-30)
        mid = (A + B) / 2 + outward * edge * 0.2
        out.append(segments_of(rtx, mid + nn * edge * 3, mid - nn * edge * 3, R))                    # beside edge AB, both endpoints far
        out.append(segments_of(rtx, C + up * 0.3 - along, C + up * 0.3 + along, R))                  # over a vertex
        out.append(segments_of(rtx, A + up * 0.1, B + up * 0.1, R))                                  # along an edge
        out.append(segments_of(rtx, B, C, R))                                                        # an edge itself
        out.append(segments_of(rtx, A, A, R))                                                        # a vertex, as a point
    if len(s):
        c, r = np.asarray(s["position"], np.float64), np.asarray(s["radius"], np.float64)[:, None]
        k = min(len(s), per_kind)
        u = rng.standard_normal((k, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = np.cross(u, rng.standard_normal((k, 3)))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        Rs = (r[:k, 0] * 2).astype(np.float32)
        out.append(segments_of(rtx, c[:k] - u * r[:k] * 2, c[:k] + u * r[:k] * 2, Rs))               # through the centre
        out.append(segments_of(rtx, c[:k] + w * r[:k] * 0.3, c[:k] + u * r[:k] * 0.5, Rs))           # inside the solid ball
        out.append(segments_of(rtx, c[:k] + w * r[:k] * 1.5 - u * r[:k], c[:k] + w * r[:k] * 1.5 + u * r[:k], Rs))   # beside it
        out.append(segments_of(rtx, c[:k] + u * r[:k] * 3, c[:k] + u * r[:k] * 1.25, Rs))            # an endpoint nearest
    mid = (lo + hi) / 2
    out.append(segments_of(rtx, [lo - ext * 0.1, mid], [hi + ext * 0.1, mid + ext * 0.01], [np.inf, 1e-30]))
    # (P0 + d = +inf with P0 and d finite is not searched either; it is not here, because a finite P0 of 3e38 with tMax > 0 enters the
    # origin bound and would widen every box of the tree beyond all culling for the whole batch: tests/test_capsule_cpu.py and
    # test_gpu_capsule.py's origin-bound test hold it)
    bad = segments_of(rtx, np.repeat(mid[None], 7, 0), np.repeat((mid + ext * 0.1)[None], 7, 0), diag)
    bad["tMax"][:3] = (0.0, -1.0, np.nan)
    bad["origin"][3, 1] = np.nan
    bad["direction"][4, 2] = np.nan
    bad["direction"][5, 0] = np.inf
    bad["origin"][6, 0] = -np.inf
    out.append(bad)
    return np.concatenate(out)


# ---- the float64 twin by another route: the distance from x(s) to a triangle is convex in s; golden section, no sub-candidates ---------------
def _point_tri64(x, A, B, C):
    """float64 distance^2 from points x (k, 3) to ONE triangle: the minimum over the plane projection, where inside, and the three edges"""
    def seg(P, d):
        dd = float(d @ d)
        tt = np.clip(((x - P) @ d) / dd, 0.0, 1.0) if dd > 0 else np.zeros(len(x))
        e = x - (P + tt[:, None] * d)
        return (e * e).sum(1)
    best = np.minimum(np.minimum(seg(A, B - A), seg(A, C - A)), seg(B, C - B))
    n = np.cross(B - A, C - A)
    nn = float(n @ n)
    if nn > 0:
        ap = x - A
        u = (np.cross(ap, C - A) @ n) / nn
        v = (np.cross(B - A, ap) @ n) / nn
        h = ap @ n
        best = np.where((u >= 0) & (v >= 0) & (u + v <= 1), np.minimum(best, h * h / nn), best)
    return best


def twin_key64(p0, d, A, B, C, iterations=90):
    """(k, s): the float64 minimum over s in [0, 1] of the squared distance from p0 + d s to the triangle, by golden section after a scan
    of 65 samples that brackets the minimum (the function is convex, so one bracket holds it)"""
    p0, d, A, B, C = (np.asarray(a, np.float64) for a in (p0, d, A, B, C))
    f = lambda ss: _point_tri64(p0 + np.atleast_1d(ss)[:, None] * d, A, B, C)        # noqa: E731
    grid = np.linspace(0.0, 1.0, 65)
    i = int(f(grid).argmin())
    a, b = grid[max(i - 1, 0)], grid[min(i + 1, 64)]
    g = (np.sqrt(5.0) - 1) / 2
    for _ in range(iterations):
        c1, c2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = f(np.array([c1, c2]))
        if f1 <= f2:
            b = c2
        else:
            a = c1
    ends = np.array([a, b, (a + b) / 2, 0.0, 1.0])
    fe = f(ends)
    j = int(fe.argmin())
    return float(fe[j]), float(ends[j])
