"""The checker of the sphere casts: tests/sweep_oracle.c bound with ctypes, the batch the GPU tests and the CPU tests share, and a
float64 numpy restatement of the definition written from the text of include/rt.h.  Test infrastructure only."""
import ctypes

import numpy as np

import closest_check as cc
from checker_build import compile_checker

GUARD = np.float32(1.0 + 2.0 ** -6)         # g = r * GUARD (include/rt.h "sphere casts")
RADII = (0.01, 0.1, 0.5)                    # of the scene's extent
N_AIMED, N_PARALLEL, N_INSIDE, N_FAR, N_UNTRACED = 560, 64, 64, 16, 6

_lib = None


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("sweep_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        so.sw_cast.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp]
        so.sw_cast.restype = ci
        _lib = so
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def rays_of(rtx, origin, direction, radius, t_max=np.inf):
    """RAY (n,): origins and directions (n, 3), the radius (a scalar or (n,)) as the bits of _reserved"""
    origin = np.asarray(origin, np.float32).reshape(-1, 3)
    r = np.zeros(len(origin), rtx.RAY)
    r["origin"], r["direction"], r["tMax"] = origin, np.asarray(direction, np.float32).reshape(-1, 3), t_max
    r["_reserved"] = np.broadcast_to(np.asarray(radius, np.float32), (len(origin),)).copy().view(np.int32)
    return r


def radii_of(rays):
    return np.ascontiguousarray(rays["_reserved"]).view(np.float32)


def oracle_cast(rtx, spheres, tris, infos, rays, chunk_mesh=None, second=False):
    """(HIT (n,), uint8 (n,)): the brute-force sphere cast of every ray and its occlusion byte; second: also float32 (n,), the time of
    the best candidate of another primitive"""
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    cm = None if chunk_mesh is None else np.ascontiguousarray(chunk_mesh, np.int32)
    assert cm is None or len(cm) == len(m)
    out, occ, sec = np.zeros(len(r), rtx.HIT), np.zeros(len(r), np.uint8), np.zeros(len(r), np.float32)
    rc = lib().sw_cast(_p(s), len(s), _p(t), len(t), _p(m), len(m), _p(cm), _p(r), len(r), _p(out), _p(occ), _p(sec))
    assert rc == 0, f"sw_cast failed: {rc}"
    return (out, occ, sec) if second else (out, occ)


def assert_same_records(rtx, got, want, what):
    """every field of every record bit for bit (NaN equal to NaN where the bits agree: the records are compared as words)"""
    got, want = np.ascontiguousarray(got, rtx.HIT).reshape(-1), np.ascontiguousarray(want, rtx.HIT).reshape(-1)
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


def scene_box(s, t, m):
    """(live triangle indices, centre, extent): extent = the half diagonal of the bounding box, at least 0.5"""
    live = np.concatenate([np.arange(i["firstTriangleIndex"], i["firstTriangleIndex"] + i["numTriangles"]) for i in m]) if len(m) else np.zeros(0, int)
    corners = [np.asarray(t[k][live], np.float64).reshape(-1, 3) for k in ("posA", "posB", "posC")] if len(live) else []
    if len(s):
        c, r = np.asarray(s["position"], np.float64), np.asarray(s["radius"], np.float64)[:, None]
        corners += [c - r, c + r]
    allp = np.concatenate(corners)
    lo, hi = allp.min(0), allp.max(0)
    return live, (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 0.5)


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def batch_of(rtx, s, t, m, seed=1):
    """(RAY (710,), classes (710,)) for a scene.  Classes: 0 = N_AIMED rays from random points on the sphere of 2 extents around the
    scene, aimed at vertices, edge midpoints and centroids of up to 40 triangles (and at sphere centres), every second one past its
    target by up to five extents so that about half of them miss; 1 = N_PARALLEL rays parallel to picked edges at offset r from the edge, in
    the triangle's plane (the edge quadratic's cancellation case); 2 = N_INSIDE rays that start within r of the geometry; 3 = N_FAR rays
    from 1e4 extents away; 4 = six that are not traced (tMax 0, -1, NaN; r 0, -1, NaN).  r cycles through RADII x extent; directions
    are not normalised (lengths 0.5 .. 2)."""
    rng = np.random.default_rng(seed)
    live, mid, ext = scene_box(s, t, m)
    targets = []
    if len(live):
        pick = live[rng.permutation(len(live))[:40]]
        A, B, C = (np.asarray(t[k][pick], np.float64) for k in ("posA", "posB", "posC"))
        targets += [A, B, C, (A + B) / 2, (A + C) / 2, (B + C) / 2, (A + B + C) / 3]
    if len(s):
        c = np.asarray(s["position"], np.float64)
        c = c[rng.permutation(len(c))[:40]]
        targets.append(np.resize(c, (max(len(c), 7 * len(live[:40]) // 3), 3)))      # at least a quarter of the targets
    targets = np.concatenate(targets)
    radius = lambda n: np.resize(np.asarray(RADII) * ext, n)       # noqa: E731
    # aimed
    tg = targets[np.arange(N_AIMED) % len(targets)].copy()
    tg[1::2] += _unit(rng, len(tg[1::2])) * rng.random((len(tg[1::2]), 1)) * 5 * ext
    o0 = mid + _unit(rng, N_AIMED) * 2 * ext
    d0 = (tg - o0) / np.linalg.norm(tg - o0, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (N_AIMED, 1))
    r0 = radius(N_AIMED)
    # parallel to an edge, at offset r in the triangle's plane, starting an edge length before it
    r1 = radius(N_PARALLEL)
    if len(live):
        k = live[rng.integers(0, len(live), N_PARALLEL)]
        P, Q, R_ = (np.asarray(t[n_][k], np.float64) for n_ in ("posA", "posB", "posC"))
        e = Q - P
        el = np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
        n = np.cross(e, R_ - P)
        out = np.cross(e, n)                                        # in the plane, away from the third corner
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-30)
        o1 = P - e + out * r1[:, None]
        d1 = e / el * rng.uniform(0.5, 2.0, (N_PARALLEL, 1))
    else:
        o1 = mid + _unit(rng, N_PARALLEL) * 2 * ext
        d1 = _unit(rng, N_PARALLEL)
    # starting inside the inflated geometry: within r of a target
    r2 = radius(N_INSIDE)
    o2 = targets[rng.integers(0, len(targets), N_INSIDE)] + _unit(rng, N_INSIDE) * (rng.random((N_INSIDE, 1)) * r2[:, None])
    d2 = _unit(rng, N_INSIDE) * rng.uniform(0.5, 2.0, (N_INSIDE, 1))
    # far away
    u3 = _unit(rng, N_FAR)
    o3 = mid + u3 * 1e4 * ext
    tg3 = targets[rng.integers(0, len(targets), N_FAR)]
    d3 = (tg3 - o3) / np.linalg.norm(tg3 - o3, axis=1, keepdims=True)
    r3 = radius(N_FAR)
    # not traced
    o4, d4, r4 = np.repeat(o0[:1], N_UNTRACED, 0), np.repeat(d0[:1], N_UNTRACED, 0), np.full(N_UNTRACED, RADII[1] * ext)
    rays = rays_of(rtx, np.concatenate([o0, o1, o2, o3, o4]), np.concatenate([d0, d1, d2, d3, d4]), np.concatenate([r0, r1, r2, r3, r4]))
    rays["tMax"][-6:-3] = (0.0, -1.0, np.nan)
    rays["_reserved"][-3:] = np.array([0.0, -1.0, np.nan], np.float32).view(np.int32)
    classes = np.repeat(np.arange(5), (N_AIMED, N_PARALLEL, N_INSIDE, N_FAR, N_UNTRACED))
    return rays, classes


def feature_class(hits):
    """per record: 0 miss, 1 scene sphere, 2 face, 3 edge, 4 vertex"""
    f = hits["_reserved"][:, 0]
    return np.where(hits["kind"] == 0, 0, np.where(hits["kind"] == 1, 1, np.where(f <= 2, 2, np.where(f <= 5, 3, 4))))


# ---- the float64 twin: include/rt.h's text again, in numpy float64, one ray against all primitives -------------------------------------
def _near_root(a, b, c):
    """the near root of a t^2 + b t + c with RaySphere's acceptance (disc >= 0, root >= 0); +inf otherwise"""
    with np.errstate(all="ignore"):
        disc = b * b - 4 * a * c
        t = (-b - np.sqrt(np.where(disc >= 0, disc, 0.0))) / (2 * a)
        return np.where((disc >= 0) & (t >= 0), t, np.inf)


def twin64(o, d, t_max, r, sphere_c, sphere_r, A, B, C):
    """(t, kind, prim, feature, point) arrays of every accepted candidate with t < tMax, sorted by (t, kind, prim, feature): spheres
    (centres (ns, 3), radii (ns,)) and the triangles (A, B, C (nt, 3)) with their seven features and the guard, all in float64"""
    o, d, r = np.asarray(o, np.float64), np.asarray(d, np.float64), float(r)
    ts, kinds, prims, feats, points = [], [], [], [], []
    dd = d @ d
    g2 = (r * float(GUARD)) ** 2

    def offer(t, kind, prim, feat, point):
        ok = np.isfinite(t) & (t < t_max)
        ts.append(t[ok]); kinds.append(np.full(ok.sum(), kind)); prims.append(prim[ok]); feats.append(np.full(ok.sum(), feat)); points.append(point[ok])

    if len(sphere_c):
        sc = np.asarray(sphere_c, np.float64)
        oc = o - sc
        t = _near_root(dd, 2 * oc @ d, (oc * oc).sum(1) - (np.asarray(sphere_r, np.float64) + r) ** 2)
        with np.errstate(all="ignore"):
            c = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
            nrm = (c - sc) / np.linalg.norm(c - sc, axis=1, keepdims=True)
        offer(t, 1, np.arange(len(sc)), 0, c - nrm * r)
    if len(A):
        A, B, C = (np.asarray(x, np.float64) for x in (A, B, C))
        idx = np.arange(len(A))
        ab, ac = B - A, C - A
        n = np.cross(ab, ac)
        with np.errstate(all="ignore"):
            N = n / np.linalg.norm(n, axis=1, keepdims=True)
            cand = []
            for code, sign in ((1, -1.0), (2, 1.0)):
                o2 = o + N * (sign * r)
                det = -(n @ d)
                ao = o2 - A
                dao = np.cross(ao, d)
                t = (ao * n).sum(1) / det
                u = (ac * dao).sum(1) / det
                v = -(ab * dao).sum(1) / det
                ok = (t >= 0) & (u >= 0) & (v >= 0) & (1 - u - v >= 0) & ((det >= 1e-6) if code == 1 else (det <= -1e-6))
                cand.append((code, np.where(ok, t, np.inf), o2 + d * np.where(ok, t, 0.0)[:, None]))
            for code, P, e in ((3, A, ab), (4, A, ac), (5, B, ac - ab)):
                m = o - P
                ee, md, nd = (e * e).sum(1), (m * e).sum(1), e @ d
                qa, qb, qc = ee * dd - nd * nd, ee * (m @ d) - nd * md, ee * ((m * m).sum(1) - r * r) - md * md
                disc = qb * qb - qa * qc
                t = (-qb - np.sqrt(np.where(disc >= 0, disc, 0.0))) / qa
                s = md + t * nd
                ok = (qa > 0) & (disc >= 0) & (t >= 0) & (s > 0) & (s < ee)
                cand.append((code, np.where(ok, t, np.inf), P + e * np.where(ok, s / ee, 0.0)[:, None]))
            for code, P in ((6, A), (7, B), (8, C)):
                oc = o - P
                cand.append((code, _near_root(dd, 2 * oc @ d, (oc * oc).sum(1) - r * r), P))
            for code, t, point in cand:
                fin = np.isfinite(t)
                k = np.full(len(A), np.inf)
                if fin.any():
                    # the guard: the ball at its time touches the triangle
                    k[fin] = cc._tri_keys64(o + d * t[fin, None], A[fin], B[fin], C[fin])
                offer(np.where(k <= g2, t, np.inf), 2, idx, code, point)
    if not ts:
        return np.zeros(0), np.zeros(0, int), np.zeros(0, int), np.zeros(0, int), np.zeros((0, 3))
    t, kind, prim, feat, point = (np.concatenate(x) for x in (ts, kinds, prims, feats, points))
    order = np.lexsort((feat, prim, kind, t))
    return t[order], kind[order], prim[order], feat[order], point[order]
