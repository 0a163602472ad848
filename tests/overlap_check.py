"""The checker of the box overlap queries: tests/overlap_oracle.c bound with ctypes, and what the overlap tests share — the batch of
boxes every scene gets (module-level `batch_of`).  The binding's one call, the word-for-word comparison, the counts and the scene's
bounds are listed_check.py's, shared with nearest_check.py and capsule_check.py.  Test infrastructure only."""
import ctypes

import numpy as np

import closest_check as cc
from checker_build import compile_checker
from listed_check import (COUNT_WORD, _live, _p, assert_same_records, bind_listed, counts, different, oracle_listed,   # noqa: F401
                          scene_bounds, words)

_lib = None

# overlap_oracle.c's `variant`: the definition and its one-line mutants
DEFINITION, BOUNDS_ONLY, NO_PLANE, NO_EDGES, OPEN_SETS, NAN_COUNTS = range(6)
MUTANTS = {"stops after the bounds": BOUNDS_ONLY, "no plane axis": NO_PLANE, "no edge axes": NO_EDGES, "open sets": OPEN_SETS,
           "a NaN key counts": NAN_COUNTS}
FORMS = ((2, 0), (8, 0), (3, 1), (1, 1))            # (K, all) of the GPU tests


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("overlap_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        bind_listed(so.ov_overlap)
        so.ov_touches.argtypes = [vp, ci, vp, ci, vp, ci, ci, vp]
        so.ov_touches.restype = ci
        _lib = so
    return _lib


def boxes_of(rtx, centres, half_extents, gate=1.0):
    """RAY (n,): origin = the centres (n, 3), direction = the half-extents (one (3,) for all, a scalar, or (n, 3)), tMax = the gate"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    b = np.zeros(len(c), rtx.RAY)
    b["origin"] = c
    b["direction"] = np.broadcast_to(np.asarray(half_extents, np.float32), c.shape) if np.ndim(half_extents) else np.float32(half_extents)
    b["tMax"] = gate
    return b


def oracle_overlap(rtx, spheres, tris, infos, boxes, k, count_all=0, chunk_mesh=None, variant=DEFINITION, totals=None, kth_ties=None):
    """CLOSEST (n, k): the brute-force answer for every box.  totals / kth_ties: int32 (n,) arrays that receive, per box, the number of
    all candidates that count and whether the k-th and (k+1)-th keys of the full sort are bit-equal"""
    return oracle_listed(lib().ov_overlap, rtx, spheres, tris, infos, boxes, k, count_all, chunk_mesh, variant, totals, kth_ties)


def oracle_touches(rtx, spheres, tris, boxes, variant=DEFINITION):
    """uint8 (n, ns + nt): the checker's touch decision of every box against every sphere, then every triangle in uploaded order"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    r = np.ascontiguousarray(boxes, rtx.RAY).reshape(-1)
    out = np.zeros((len(r), len(s) + len(t)), np.uint8)
    assert lib().ov_touches(_p(s), len(s), _p(t), len(t), _p(r), len(r), int(variant), _p(out)) == 0
    return out


# ---- the batch ------------------------------------------------------------------------------------------------------------------------------
def batch_of(rtx, s, t, m, base, seed=17, per_kind=24):
    """the scene's own closest-point batch `base` (test_gpu_closest.batch_of) read as boxes of a half-extent comparable to the scene's
    triangles, and appended to it, per kind up to `per_kind` boxes built on triangles picked at random:
      * boxes that contain a whole triangle (its bounds, inflated);
      * boxes pierced by a triangle's interior with no vertex inside: a small cube at the centroid — only the plane axis can reject it,
        and a thin slab just off the plane, which it must reject;
      * boxes whose bounds overlap the triangle's bounds while an edge axis separates them: a small cube in the corner of the triangle's
        bounds that lies opposite its longest edge's far side (a kernel that stops after the bounds condition reports these);
      * boxes whose face coordinate equals a vertex's coordinate bit for bit (hi = the vertex on one axis): touching counts, and where
        the vertex is shared the keys of its triangles tie;
      * h = 0 on a surface (a vertex, a centroid) and h = 0 off it;
      * two boxes 3e19 off the scene with half-extents 4e19: everything touches, every key is +inf;
      * one box over the whole scene; a box that touches nothing;
      * inputs that are not searched: tMax 0, negative, NaN; a negative, NaN and infinite half-extent; a NaN centre."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(s, t, m)
    ext = np.maximum(hi - lo, 1e-3)
    live = _live(m)
    out = []
    p = np.ascontiguousarray(base, rtx.RAY).copy()
    if len(live):
        A, B, C = (np.asarray(t[k][live], np.float64) for k in ("posA", "posB", "posC"))
        size = float(np.median(np.maximum(np.abs(B - A), np.abs(C - A)).max(1)))
    else:
        size = float(np.median(s["radius"]))
    p["direction"] = (rng.uniform(0.25, 1.5, (len(p), 3)) * size).astype(np.float32)
    p["tMax"] = np.where(p["tMax"] > 0, np.float32(1.0), p["tMax"])            # (a gate only; the three unsearched points stay)
    out.append(p)
    if len(live):
        pick = live[rng.permutation(len(live))[:per_kind]]
        A, B, C = (np.asarray(t[k][pick], np.float32) for k in ("posA", "posB", "posC"))
        mn, mx = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
        mid, half = (mn + mx) / 2, (mx - mn) / 2
        edge = np.maximum(half.max(1, keepdims=True), 1e-6)
        cen = ((A.astype(np.float64) + B + C) / 3).astype(np.float32)
        out.append(boxes_of(rtx, mid, half * 1.25 + edge * 0.01))                                   # contains the whole triangle
        out.append(boxes_of(rtx, cen, edge * 0.05))                                                 # pierced, no vertex inside
        n = np.cross(B - A.astype(np.float64), C - A.astype(np.float64))
        nn = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        thin = np.maximum(edge * 0.3 * (1 - np.abs(nn)), edge * 0.01)
        out.append(boxes_of(rtx, cen + (nn * edge * 0.08).astype(np.float32), thin.astype(np.float32)))    # a slab beside the plane
        # the corner of the bounds farthest from the triangle: inside its bounds, outside the triangle unless it is axis-aligned
        corners = np.stack([np.where([(i >> a) & 1 for a in range(3)], mx, mn) for i in range(8)], 1)         # (n, 8, 3)
        far = np.array([[cc._tri_keys64(corners[j, i].astype(np.float64), A[j:j + 1].astype(np.float64), B[j:j + 1].astype(np.float64),
                                        C[j:j + 1].astype(np.float64))[0] for i in range(8)] for j in range(len(pick))]).argmax(1)
        corner = corners[np.arange(len(pick)), far]
        inward = np.sign(mid - corner).astype(np.float32)
        out.append(boxes_of(rtx, corner + inward * edge * 0.06, edge * 0.05))                      # bounds overlap, an edge axis separates
        # a face on a vertex, bit for bit: hi.x = A.x exactly needs c + h == A.x in float32 — h a power of two, c = A.x - h when exact
        h2 = np.float32(2.0) ** np.floor(np.log2(edge))
        for V in (A, B):
            c = V.copy()
            c[:, 0] = V[:, 0] - h2[:, 0]
            ok = (c[:, 0] + h2[:, 0]) == V[:, 0]
            out.append(boxes_of(rtx, c[ok], np.repeat(h2[ok], 3, 1)))
        out.append(boxes_of(rtx, np.concatenate([A[:8], cen[:8]]), 0.0))                            # h = 0 on a surface
        out.append(boxes_of(rtx, cen[:8] + (nn[:8] * edge[:8] * 0.5).astype(np.float32), 0.0))      # h = 0 off it
    if len(s):
        c, r = np.asarray(s["position"], np.float32), np.asarray(s["radius"], np.float32)[:, None]
        k = min(len(s), per_kind)
        d = rng.standard_normal((k, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(boxes_of(rtx, c[:k], r[:k] * 0.25))                                              # inside the solid ball
        out.append(boxes_of(rtx, c[:k] + d * r[:k] * 1.3, r[:k] * 0.2))                             # near the surface, either way
        face = c[:k].copy()
        face[:, 0] += r[:k, 0] * 2                                                                  # lo.x = c.x + r where that is exact
        out.append(boxes_of(rtx, face, r[:k]))
        out.append(boxes_of(rtx, c[:4] + d[:4] * r[:4], 0.0))
    mid = ((lo + hi) / 2).astype(np.float32)
    # far off-centre and large: it still reaches every surface, and every key, |c - q|^2 near 9e38, overflows to +inf — the candidates
    # tie with each other and with the list's empty slots
    out.append(boxes_of(rtx, [mid + np.float32([3e19, 0, 0]), mid + np.float32([0, -3e19, 3e19])], np.float32(4e19)))
    out.append(boxes_of(rtx, [mid], (ext * 0.75).astype(np.float32)))                               # the whole scene
    out.append(boxes_of(rtx, [mid + (ext * 4).astype(np.float32)], (ext * 0.5).astype(np.float32)))  # nothing
    bad = boxes_of(rtx, np.repeat(mid[None], 7, 0), (ext * 0.75).astype(np.float32))
    bad["tMax"][:3] = (0.0, -1.0, np.nan)
    bad["direction"][3, 1] = -1e-3
    bad["direction"][4, 2] = np.nan
    bad["direction"][5, 0] = np.inf
    bad["origin"][6, 1] = np.nan
    out.append(bad)
    return np.concatenate(out)
