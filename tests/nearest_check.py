"""The checker of the K-nearest point queries: tests/nearest_oracle.c bound with ctypes, and what the K-nearest tests share — the batches
whose points tie at the K-th key, the float64 twin's sorted distances.  The binding's one call, the word-for-word comparison and the
count word are listed_check.py's, shared with overlap_check.py and capsule_check.py.  Test infrastructure only."""
import numpy as np

import closest_check as cc
from checker_build import compile_checker
from listed_check import (COUNT_WORD, _live, assert_first_is_the_default, assert_same_records, bind_listed, different,   # noqa: F401
                          oracle_listed, words)

_lib = None

# nearest_oracle.c's `variant`: the definition and its one-line mutants
DEFINITION, NON_STRICT, TIE_BY_POSITION, TRIANGLE_FIRST, COUNT_CAPPED, DROPS_EQUAL = range(6)
MUTANTS = {"non-strict radius": NON_STRICT, "tie by position": TIE_BY_POSITION, "triangle before sphere": TRIANGLE_FIRST,
           "count capped at K": COUNT_CAPPED, "drops k == kth": DROPS_EQUAL}
FORMS = ((2, 0), (8, 0), (3, 1), (1, 1))            # (K, all) of the GPU tests


def lib(directory=None):
    global _lib
    if _lib is None:
        _lib = compile_checker("nearest_oracle.c", directory)
        bind_listed(_lib.np_nearest)
    return _lib


def oracle_nearest(rtx, spheres, tris, infos, points, k, count_all=0, chunk_mesh=None, variant=DEFINITION, totals=None, kth_ties=None):
    """CLOSEST (n, k): the brute-force answer for every point.  totals / kth_ties: int32 (n,) arrays that receive, per point, the number of
    all candidates below R * R and whether the k-th and (k+1)-th keys of the full sort are bit-equal"""
    return oracle_listed(lib().np_nearest, rtx, spheres, tris, infos, points, k, count_all, chunk_mesh, variant, totals, kth_ties)


def tie_plane(rtx, n=16, spacing=2.0):
    """test_gpu_closest.plane's tessellation, restated with a dyadic spacing: 2 n^2 triangles over [0, n * spacing]^2 at z = 0, vertices
    on multiples of `spacing` — A + (B - A) == B exactly, so the six triangles around an inner vertex give bit-equal keys"""
    xs = np.arange(n + 1, dtype=np.float32) * np.float32(spacing)
    t = np.zeros(2 * n * n, rtx.TRIANGLE)
    k = 0
    for j in range(n):
        for i in range(n):
            a, b, c, d = (xs[i], xs[j], 0), (xs[i + 1], xs[j], 0), (xs[i + 1], xs[j + 1], 0), (xs[i], xs[j + 1], 0)
            t["posA"][k], t["posB"][k], t["posC"][k] = a, b, c
            t["posA"][k + 1], t["posB"][k + 1], t["posC"][k + 1] = a, c, d
            k += 2
    t["normalA"] = t["normalB"] = t["normalC"] = (0, 0, 1)
    m = np.zeros(1, rtx.MESHINFO)
    m["numTriangles"] = len(t)
    m["boundsMin"], m["boundsMax"] = (0, 0, 0), (n * spacing, n * spacing, 0)
    return np.zeros(0, rtx.SPHERE), t, m


def around_vertex(n, i, j):
    """the uploaded indices of the six triangles of tie_plane / plane(rtx, n, n) that meet at inner vertex (i, j), ascending"""
    cell = lambda ci, cj: 2 * (cj * n + ci)      # noqa: E731
    # cell (i-1, j-1): both triangles (corner c); cell (i, j-1): the second (corner d); cell (i-1, j): the first (corner b); cell (i, j): both (a)
    return sorted([cell(i - 1, j - 1), cell(i - 1, j - 1) + 1, cell(i, j - 1) + 1, cell(i - 1, j), cell(i, j), cell(i, j) + 1])


def vertex_tie_points(rtx, s, t, m, count=128, seed=11):
    """`count` points straight above (or on) vertices of the scene's triangles, at dyadic heights, with a radius that takes in more than
    eight candidates where the scene has them: the points whose K-th and (K+1)-th keys tie wherever several triangles share the vertex"""
    live = _live(m)
    if not len(live):
        return cc.points_of(rtx, np.zeros((0, 3)))
    rng = np.random.default_rng(seed)
    pick = live[rng.integers(0, len(live), count)]
    corner = rng.integers(0, 3, count)
    v = np.stack([np.asarray(t[k][pick], np.float32) for k in ("posA", "posB", "posC")], 1)[np.arange(count), corner]
    normal = np.cross(np.asarray(t["posB"][pick], np.float64) - t["posA"][pick], np.asarray(t["posC"][pick], np.float64) - t["posA"][pick])
    axis = np.abs(normal).argmax(1)
    edge = np.linalg.norm(np.asarray(t["posB"][pick], np.float64) - t["posA"][pick], axis=1)
    h = np.float32(2.0) ** np.floor(np.log2(np.maximum(edge, 1e-6)) - rng.integers(0, 3, count))
    xyz = v.copy()
    xyz[np.arange(count), axis] += np.where(rng.random(count) < 0.25, 0, h).astype(np.float32)
    return cc.points_of(rtx, xyz, (4 * np.maximum(edge, h)).astype(np.float32))


def batch_of(rtx, s, t, m, base):
    """a closest-point batch `base` (test_gpu_closest.batch_of: its three unsearched points last) with half its searched points given a
    finite radius and the vertex-tie points put in front"""
    p = np.ascontiguousarray(base, rtx.RAY).copy()
    finite = np.isfinite(p["origin"]).all(1)
    if len(t) or len(s):
        lo = np.minimum(t["posA"].min(0) if len(t) else np.inf, (s["position"] - s["radius"][:, None]).min(0) if len(s) else np.inf)
        hi = np.maximum(t["posA"].max(0) if len(t) else -np.inf, (s["position"] + s["radius"][:, None]).max(0) if len(s) else -np.inf)
        R = np.float32(np.linalg.norm(hi - lo) / 4)
        half = np.flatnonzero(finite & (p["tMax"] > 0))[::2]
        p["tMax"][half] = R
    return np.concatenate([vertex_tie_points(rtx, s, t, m), p])


def twin_sorted_dst(p, R, sphere_c, sphere_r, A, B, C):
    """float64: the distances of ALL candidates of point p, ascending (closest_check.twin64's keys without the radius), for the j-th
    smallest distance and the counts on either side of R"""
    k = cc.twin64(p, np.inf, sphere_c, sphere_r, A, B, C)[0]
    return np.sqrt(k)
