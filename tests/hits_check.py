"""The checker of the multi-hit ray queries: tests/hits_oracle.c bound with ctypes, a float64 numpy restatement of the same definition
written from the text of include/rt.h, and what the multi-hit tests share — the scenes, and the batch generator that the CPU tests
(which cap the tie rays) and the GPU tests (which trace them) both draw from.  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

FRONT, BOTH = 0, 1
SCENES = ("one", "two", "plane", "spheres", "mixed", "Knight", "Suzanne", "layers", "shells")
_lib = None


def lib(directory=None):
    global _lib
    if _lib is None:
        so = compile_checker("hits_oracle.c", directory)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        so.mh_trace.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, vp]
        so.mh_all.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, ci]
        so.mh_trace.restype = so.mh_all.restype = ci
        _lib = so
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _scene(rtx, spheres, tris, infos, chunk_mesh):
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    cm = None if chunk_mesh is None else np.ascontiguousarray(chunk_mesh, np.int32)
    assert cm is None or len(cm) == len(m)
    return [_p(s), len(s), _p(t), len(t), _p(m), len(m), _p(cm)], (s, t, m, cm)


def oracle_hits(rtx, spheres, tris, infos, rays, K=4, mode=FRONT, count_all=False, intersect=0, chunk_mesh=None):
    """MULTIHIT (n, K): the brute-force answer for every ray"""
    sc, _keep = _scene(rtx, spheres, tris, infos, chunk_mesh)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    out = np.zeros((len(r), K), rtx.MULTIHIT)
    rc = lib().mh_trace(*sc, int(intersect), _p(r), len(r), int(K), int(mode), int(bool(count_all)), _p(out))
    assert rc == 0, f"mh_trace failed: {rc}"
    return out


def oracle_all(rtx, spheres, tris, infos, ray, mode=FRONT, intersect=0, chunk_mesh=None):
    """MULTIHIT (total,): every hit of ONE ray below its tMax, in order (hitCount = total in each)"""
    sc, _keep = _scene(rtx, spheres, tris, infos, chunk_mesh)
    r = np.ascontiguousarray(ray, rtx.RAY).reshape(-1)[:1]
    cap = 2 * sc[1] + sc[3] + 1
    out = np.zeros(cap, rtx.MULTIHIT)
    total = lib().mh_all(*sc, int(intersect), _p(r), int(mode), _p(out), cap)
    assert total >= 0, f"mh_all failed: {total}"
    return out[:total]


def make_rays(rtx, origins, directions, t_max=np.inf):
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    r = np.zeros(len(o), rtx.RAY)
    r["origin"], r["direction"], r["tMax"] = o, np.asarray(directions, np.float32).reshape(-1, 3), t_max
    return r


FLOAT_WORDS = [0, 1, 2, 3, 4, 5, 6, 11, 12]      # of a MULTIHIT record's sixteen


def assert_same_records(rtx, got, want, what):
    """every field of every record bit for bit (NaN equal to NaN where both are: the records are compared as words)"""
    got, want = np.ascontiguousarray(got, rtx.MULTIHIT), np.ascontiguousarray(want, rtx.MULTIHIT)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1).view(np.uint32).reshape(-1, 16), want.reshape(-1).view(np.uint32).reshape(-1, 16)
    gf, wf = g.view(np.float32), w.view(np.float32)
    is_float = np.zeros(16, bool)
    is_float[FLOAT_WORDS] = True
    same = (g == w) | (is_float[None, :] & np.isnan(gf) & np.isnan(wf))
    if not same.all():
        rows = np.flatnonzero(~same.all(1))
        i = int(rows[0])
        K = got.shape[-1] if got.ndim == 2 else 1
        raise AssertionError(f"{what}: {len(rows)} of {len(g)} records differ; first at ray {i // K} record {i % K}:\n"
                             f" got  {got.reshape(-1)[i]!r}\n want {want.reshape(-1)[i]!r}")


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _quads(rtx, z, flip, n=4, size=4.0):
    """2 n^2 triangles tessellating [0, size]^2 at height z, normals +z (flip: the other winding, normals -z)"""
    xs = np.linspace(0, size, n + 1, dtype=np.float32)
    t = np.zeros(2 * n * n, rtx.TRIANGLE)
    k = 0
    for j in range(n):
        for i in range(n):
            a, b, c, d = (xs[i], xs[j], z), (xs[i + 1], xs[j], z), (xs[i + 1], xs[j + 1], z), (xs[i], xs[j + 1], z)
            for tri in ((a, b, c), (a, c, d)):
                A, B, C = tri if not flip else (tri[0], tri[2], tri[1])
                t["posA"][k], t["posB"][k], t["posC"][k] = A, B, C
                k += 1
    t["normalA"] = t["normalB"] = t["normalC"] = (0, 0, -1 if flip else 1)
    return t


def layers(rtx, planes=12):
    """12 parallel planes of 4 x 4 quads half a unit apart, every third one facing down, a chunk each: rays along z cross more than
    eight surfaces"""
    tris = [_quads(rtx, np.float32(0.5 * p), p % 3 == 2) for p in range(planes)]
    m = np.zeros(planes, rtx.MESHINFO)
    for p in range(planes):
        m["firstTriangleIndex"][p], m["numTriangles"][p] = 32 * p, 32
        m["boundsMin"][p], m["boundsMax"][p] = (0, 0, 0.5 * p), (4, 4, 0.5 * p)
    return np.zeros(0, rtx.SPHERE), np.concatenate(tris), m


def _cube(rtx, centre, half):
    """a closed cube of 12 triangles wound outwards, face normals at the vertices"""
    c = np.asarray(centre, np.float32)
    t = np.zeros(12, rtx.TRIANGLE)
    k = 0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3, np.float32)
            n[axis] = sign

            def corner(su, sv):
                p = np.zeros(3, np.float32)
                p[axis], p[u], p[v] = sign * half, su * half, sv * half
                return c + p
            q = [corner(-1, -1), corner(1, -1), corner(1, 1), corner(-1, 1)]
            if sign < 0:
                q = q[::-1]                                      # (u x v = +axis: the other way round for the face that looks down the axis)
            for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                t["posA"][k], t["posB"][k], t["posC"][k] = tri
                t["normalA"][k] = t["normalB"][k] = t["normalC"][k] = n
                k += 1
    return t


def shells(rtx):
    """six concentric spheres around three nested closed cubes (a chunk each): entry / exit pairs for RT_HITS_BOTH"""
    centre = (1.0, 2.0, 3.0)
    s = np.zeros(6, rtx.SPHERE)
    s["position"] = centre
    s["radius"] = [1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    halves = (0.25, 0.5, 0.75)
    t = np.concatenate([_cube(rtx, centre, h) for h in halves])
    m = np.zeros(3, rtx.MESHINFO)
    for i, h in enumerate(halves):
        m["firstTriangleIndex"][i], m["numTriangles"][i] = 12 * i, 12
        m["boundsMin"][i], m["boundsMax"][i] = np.float32(centre) - np.float32(h), np.float32(centre) + np.float32(h)
    return s, t, m


def buffers_of(rtx, name):
    """(spheres, triangles, meshinfo) of a scene of SCENES: tests/test_gpu_closest.py's seven and the two above"""
    if name == "layers":
        return layers(rtx)
    if name == "shells":
        return shells(rtx)
    import test_gpu_closest
    return test_gpu_closest.buffers_of(rtx, name)


# ---- the batch of a scene ---------------------------------------------------------------------------------------------------------------
N_RANDOM, N_TIES, N_SURFACE, N_TMAX = 2200, 40, 300, 50


def batch_of(rtx, s, t, m, seed=1):
    """The rays every multi-hit test traces through a scene, about 2900 of them:
      2200 random rays from the bounding box inflated 1.5 x towards random points of the box, directions of lengths 1/4 .. 4;
        40 aimed at vertices and edge midpoints of up to 40 triangles, and 8 axis-parallel ones through vertices (ties; they stay
           below 2 % of the batch: tests/test_hits_cpu.py caps the rays whose CLOSEST hit is a tie);
       300 with their origin on a surface (a triangle's centroid, a sphere's pole), random directions;
       300 copies of the first random rays with tMax 0, -1, NaN, 1e-6, exactly the dst of their first front hit, and the float after it;
        24 with a NaN or infinity in one component, 8 with a zero direction."""
    rng = np.random.default_rng(seed)
    live = np.concatenate([np.arange(i["firstTriangleIndex"], i["firstTriangleIndex"] + i["numTriangles"]) for i in m]) if len(m) else np.zeros(0, int)
    corners = [np.asarray(t[k][live], np.float64).reshape(-1, 3) for k in ("posA", "posB", "posC")] if len(live) else []
    if len(s):
        c, r = np.asarray(s["position"], np.float64), np.asarray(s["radius"], np.float64)[:, None]
        corners += [c - r, c + r]
    allp = np.concatenate(corners)
    lo, hi = allp.min(0), allp.max(0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)

    def unit(n):
        d = rng.standard_normal((n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    o = mid + (rng.random((N_RANDOM, 3)) * 2 - 1) * half * 1.5
    target = mid + (rng.random((N_RANDOM, 3)) * 2 - 1) * half
    d = target - o
    d *= (rng.uniform(0.25, 4.0, (N_RANDOM, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    parts = [make_rays(rtx, o, d)]
    if len(live):
        pick = live[rng.permutation(len(live))[:N_TIES]]
        A, B, C = (np.asarray(t[k][pick], np.float64) for k in ("posA", "posB", "posC"))
        aims = np.where((np.arange(len(pick)) % 2 == 0)[:, None], A, (B + C) / 2)
        oo = aims + unit(len(pick)) * np.linalg.norm(half) * rng.uniform(0.5, 2.0, (len(pick), 1))
        parts.append(make_rays(rtx, oo, aims - oo))
        ax = np.zeros((8, 3))
        ax[np.arange(8), np.arange(8) % 3] = np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
        through = np.asarray(t["posA"][live[rng.integers(0, len(live), 8)]], np.float64)
        parts.append(make_rays(rtx, through - ax * 3 * np.linalg.norm(half), ax * 0.5))
        on = live[rng.integers(0, len(live), N_SURFACE if not len(s) else N_SURFACE // 2)]
        A, B, C = (np.asarray(t[k][on], np.float32) for k in ("posA", "posB", "posC"))
        parts.append(make_rays(rtx, (A + B + C) / np.float32(3), unit(len(on))))
    if len(s):
        k = rng.integers(0, len(s), N_SURFACE if not len(live) else N_SURFACE // 2)
        pole = np.asarray(s["position"][k], np.float32).copy()
        pole[:, 1] += np.asarray(s["radius"][k], np.float32)
        parts.append(make_rays(rtx, pole, unit(len(k))))
    special = parts[0][:6 * N_TMAX].copy()
    first = oracle_hits(rtx, s, t, m, special, K=1)[:, 0]["dst"]
    for g, value in enumerate((0.0, -1.0, np.nan, 1e-6, None, None)):
        sl = slice(g * N_TMAX, (g + 1) * N_TMAX)
        if value is not None:
            special["tMax"][sl] = value
        else:
            hit = np.isfinite(first[sl])
            exact = first[sl] if g == 4 else np.nextafter(first[sl], np.float32(np.inf))
            special["tMax"][sl] = np.where(hit, exact, np.float32(0.5))
    parts.append(special)
    bad = parts[0][6 * N_TMAX:6 * N_TMAX + 32].copy()
    for i, value in enumerate((np.nan, np.inf, -np.inf) * 8):
        bad["origin" if i % 2 else "direction"][i, i % 3] = value
    bad["direction"][24:] = 0.0
    bad["direction"][28:, 0] = -0.0
    parts.append(bad)
    rays = np.concatenate(parts)
    assert 2000 <= len(rays) <= 4000
    return rays


# ---- the float64 twin: include/rt.h's text again in numpy float64, one ray against all primitives, sorted by numpy -----------------------
def twin64(o, d, t_max, sphere_c, sphere_r, A, B, C, both):
    """(dst, kind, prim, side) arrays: every hit of the ray below t_max in ascending (dst, kind, prim, front before back), float64.  No
    chunk boxes (RT_INTERSECT_BRUTE's rule)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    dst, kind, prim, side = [], [], [], []
    if len(sphere_c):
        oc = o - np.asarray(sphere_c, np.float64)
        a = d @ d
        b = 2.0 * (oc @ d)
        c = (oc * oc).sum(1) - np.asarray(sphere_r, np.float64) ** 2
        disc = b * b - 4.0 * a * c
        ok = disc >= 0
        root = np.sqrt(np.where(ok, disc, 0.0))
        for sgn, sd in ((-1.0, 1), (1.0, -1)):
            if sd == -1 and not both:
                continue
            q = (-b + sgn * root) / (2.0 * a)
            keep = ok & (q >= 0)
            dst.append(q[keep]); kind.append(np.full(keep.sum(), 1)); prim.append(np.flatnonzero(keep)); side.append(np.full(keep.sum(), sd))
    if len(A):
        A, B, C = (np.asarray(x, np.float64) for x in (A, B, C))
        eAB, eAC = B - A, C - A
        n = np.cross(eAB, eAC)
        ao = o - A
        dao = np.cross(ao, d)
        det = -(n @ d)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            q = (ao * n).sum(1) * inv
            u = (eAC * dao).sum(1) * inv
            v = -(eAB * dao).sum(1) * inv
        w = 1.0 - u - v
        inside = (q >= 0) & (u >= 0) & (v >= 0) & (w >= 0)
        front = inside & (det >= 1e-6)
        back = inside & (det <= -1e-6) & bool(both)
        for keep, sd in ((front, 1), (back, -1)):
            dst.append(q[keep]); kind.append(np.full(keep.sum(), 2)); prim.append(np.flatnonzero(keep)); side.append(np.full(keep.sum(), sd))
    if not dst:
        z = np.zeros(0, int)
        return np.zeros(0), z, z, z
    dst, kind, prim, side = (np.concatenate(x) for x in (dst, kind, prim, side))
    ok = dst < np.float64(t_max)
    dst, kind, prim, side = dst[ok], kind[ok], prim[ok], side[ok]
    order = np.lexsort((-side, prim, kind, dst))
    return dst[order], kind[order], prim[order], side[order]
