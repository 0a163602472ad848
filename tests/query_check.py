"""The checker of the four query families: tests/query_oracle.c bound with ctypes, the numpy restatements of its tree and basis, and what
the ray-query, radiance, gather and visibility tests share.  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

COSINE, SH9, DISTANCE = 0, 1, 2             # the gather modes (0, 1) and the visibility modes (0, 1, 2)
MODES = (COSINE, SH9, DISTANCE)
CHANNELS = {COSINE: 4, SH9: 10, DISTANCE: 3}    # of a visibility sample
_lib = None


def lib(directory=None):
    """tests/query_oracle.c (checker_build.compile_checker) with its argument types"""
    global _lib
    if _lib is None:
        so = compile_checker("query_oracle.c", directory)
        vp, ci, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        scene = [vp, ci, vp, ci, vp, ci]
        so.rq_trace.argtypes = scene + [ci, vp, ci, ci, vp]
        so.rq_candidates.argtypes = scene + [ci, vp, ci, vp]
        so.rad_trace.argtypes = [vp] + scene + [vp, ci, ci, u32, u32, ci, vp, vp]
        so.rad_sample.argtypes = [vp] + scene + [vp, u32, u32, u32, ci, vp]
        so.rad_camera_rays.argtypes = [vp, ci, vp]
        so.gth_gather.argtypes = [vp] + scene + [vp, ci, ci, u32, u32, ci, ci, vp, vp]
        so.gth_sample.argtypes = [vp] + scene + [vp, u32, u32, u32, ci, ci, vp]
        so.vis_gather.argtypes = scene + [ci, vp, ci, ci, u32, u32, ci, ci, vp]
        so.vis_sample.argtypes = scene + [ci, vp, u32, u32, u32, ci, ci, vp]
        so.query_direction.argtypes = [vp, u32, u32, u32, ci, vp]
        for f in (so.rq_trace, so.rq_candidates, so.rad_trace, so.rad_sample, so.rad_camera_rays, so.gth_gather, so.gth_sample,
                  so.vis_gather, so.vis_sample, so.query_direction):
            f.restype = ci
        _lib = so
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scene(rtx, spheres, tris, infos):
    """the scene arguments of every entry: (spheres, ns, triangles, nt, meshinfo, nm) and the arrays that own the memory"""
    keep = (np.ascontiguousarray(spheres, rtx.SPHERE), np.ascontiguousarray(tris, rtx.TRIANGLE), np.ascontiguousarray(infos, rtx.MESHINFO))
    return [x for a in keep for x in (_p(a), len(a))], keep


def _params(rtx, params):
    return np.array(params, dtype=rtx.PARAMS).reshape(()).copy()


def _u32(v):
    return int(v) & 0xFFFFFFFF


def oracle_hits(rtx, shim, spheres, tris, infos, mode, rays, accel=False):
    """HIT (n,): the closest hit of every ray on the CPU oracle, by its literal loop or (accel) its search tree"""
    sc, _keep = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    out = np.zeros(len(r), rtx.HIT)
    assert shim.rq_trace(*sc, int(mode), _p(r), len(r), 1 if accel else 0, _p(out)) == 0
    return out


def oracle_candidates(rtx, shim, spheres, tris, infos, mode, rays):
    """int32 (n,): the candidates at the bit-identical dst of every ray's closest hit, the winner included (0: a miss)"""
    sc, _keep = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    out = np.zeros(len(r), np.int32)
    assert shim.rq_candidates(*sc, int(mode), _p(r), len(r), _p(out)) == 0
    return out


def oracle_radiance(rtx, params, spheres, tris, infos, rays, samples, seed=0, first_index=0, accel=True, count_casts=False):
    """float32 (n, 4): the radiance query of every ray on the CPU oracle (and the casts its samples made, if asked for)"""
    p, (sc, _keep) = _params(rtx, params), _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 4), np.float32)
    casts = ctypes.c_uint64(0)
    rc = lib().rad_trace(_p(p), *sc, _p(r), len(r), int(samples), _u32(seed), _u32(first_index), 1 if accel else 0, _p(out),
                         ctypes.cast(ctypes.byref(casts), ctypes.c_void_p))
    assert rc == 0, f"rad_trace failed: {rc}"
    return (out, casts.value) if count_casts else out


def oracle_radiance_sample(rtx, params, spheres, tris, infos, ray, sample, seed=0, index=0, accel=True):
    """float32 (3,): sample `sample` alone of one ray with stream index `index`"""
    p, (sc, _keep) = _params(rtx, params), _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(ray, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(3, np.float32)
    rc = lib().rad_sample(_p(p), *sc, _p(r), int(sample), _u32(seed), _u32(index), 1 if accel else 0, _p(out))
    assert rc == 0, f"rad_sample failed: {rc}"
    return out


def frame_camera_rays(rtx, params, frame):
    """RAY (width * height,): sample 0's camera ray of every pixel of frame `frame` as frag draws it in Philox mode, in pixelIndex order"""
    p = _params(rtx, params)
    rays = np.zeros(int(p["width"]) * int(p["height"]), rtx.RAY)
    assert lib().rad_camera_rays(_p(p), int(frame), _p(rays)) == 0
    return rays


def oracle_gather(rtx, params, spheres, tris, infos, points, samples, seed=0, first_index=0, mode=COSINE, accel=True, count_casts=False):
    """float32 (n, 4) in mode 0, (n, 9, 4) in mode 1: the gather query of every point on the CPU oracle (and the casts its samples made,
    if asked for)"""
    p, (sc, _keep) = _params(rtx, params), _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 9, 4) if mode == SH9 else (len(r), 4), np.float32)
    casts = ctypes.c_uint64(0)
    rc = lib().gth_gather(_p(p), *sc, _p(r), len(r), int(samples), _u32(seed), _u32(first_index), int(mode), 1 if accel else 0, _p(out),
                          ctypes.cast(ctypes.byref(casts), ctypes.c_void_p))
    assert rc == 0, f"gth_gather failed: {rc}"
    return (out, casts.value) if count_casts else out


def oracle_gather_sample(rtx, params, spheres, tris, infos, point, sample, seed=0, index=0, mode=COSINE, accel=True):
    """float32 (3,): L of sample `sample` alone of one point with stream index `index`"""
    p, (sc, _keep) = _params(rtx, params), _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(point, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(3, np.float32)
    rc = lib().gth_sample(_p(p), *sc, _p(r), int(sample), _u32(seed), _u32(index), int(mode), 1 if accel else 0, _p(out))
    assert rc == 0, f"gth_sample failed: {rc}"
    return out


def oracle_visibility(rtx, spheres, tris, infos, points, samples, seed=0, first_index=0, mode=COSINE, intersect=0, accel=True):
    """float32 (n, 4) in modes 0 and 2, (n, 12) in mode 1: the visibility gather of every point on the CPU oracle"""
    sc, _keep = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 12 if mode == SH9 else 4), np.float32)
    rc = lib().vis_gather(*sc, int(intersect), _p(r), len(r), int(samples), _u32(seed), _u32(first_index), int(mode), 1 if accel else 0,
                          _p(out))
    assert rc == 0, f"vis_gather failed: {rc}"
    return out


def oracle_visibility_sample(rtx, spheres, tris, infos, point, sample, seed=0, index=0, mode=COSINE, intersect=0, accel=True):
    """float32 (4,), (10,) or (3,): the channels of sample `sample` alone of one (traced) point with stream index `index` — mode 0
    (v ? d : 0, v), mode 1 (v ? Y_k : 0, v), mode 2 (r, r * r, hit)"""
    sc, _keep = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(point, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(10, np.float32)
    rc = lib().vis_sample(*sc, int(intersect), _p(r), int(sample), _u32(seed), _u32(index), int(mode), 1 if accel else 0, _p(out))
    assert rc == CHANNELS[mode], f"vis_sample failed: {rc}"
    return out[:rc].copy()


def direction(normal, sample, seed=0, index=0, mode=COSINE):
    """float32 (3,): the direction of sample `sample` of a gather or visibility point with that normal and stream index"""
    n = np.ascontiguousarray(normal, np.float32).reshape(3).copy()
    out = np.empty(3, np.float32)
    assert lib().query_direction(_p(n), int(sample), _u32(seed), _u32(index), int(mode), _p(out)) == 0
    return out


def directions(rtx, points, sample, seed=0, first_index=0, mode=COSINE):
    """float32 (n, 3): sample `sample`'s direction of every point of a batch"""
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    return np.stack([direction(r["direction"][i], sample, seed, (first_index + i) & 0xFFFFFFFF, mode) for i in range(len(r))]) \
        if len(r) else np.zeros((0, 3), np.float32)


def sample_rays(rtx, points, samples, seed=0, first_index=0, mode=COSINE):
    """RAY (n * samples,): the ray (origin, the checker's direction, reach) of every sample of every point, point-major — what a caller
    without rt_visibility hands to rt_occluded / rt_trace_rays"""
    pts = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    rays = np.zeros((len(pts), samples), rtx.RAY)
    for i in range(len(pts)):
        rays["origin"][i] = pts["origin"][i]
        rays["tMax"][i] = pts["tMax"][i]
        for s in range(samples):
            rays["direction"][i, s] = direction(pts["direction"][i], s, seed, (first_index + i) & 0xFFFFFFFF, mode)
    return rays.reshape(-1)


def surface_points(rtx, hits, t_max=np.inf, offset=1e-3):
    """The points the GPU tests gather at: hitPoint + offset * normal with the normal, misses kept with origin 0 and n = 0"""
    pts = np.zeros(len(hits), rtx.RAY)
    n = np.asarray(hits["normal"], np.float32)
    pts["origin"] = (np.asarray(hits["hitPoint"], np.float32) + np.float32(offset) * n).astype(np.float32)
    pts["direction"] = n
    pts["tMax"] = t_max
    return pts


def sh_basis(d):
    """float32 (9,): the basis on d = (x, y, z) as include/rt.h writes it, every product rounded to float32"""
    f = np.float32
    x, y, z = (f(v) for v in d)
    with np.errstate(all="ignore"):
        return np.array([f(0.28209479), f(0.48860251) * y, f(0.48860251) * z, f(0.48860251) * x, f(1.09254843) * f(x * y),
                         f(1.09254843) * f(y * z), f(0.31539157) * f(f(f(3.0) * f(z * z)) - f(1.0)), f(1.09254843) * f(x * z),
                         f(0.54627421) * f(f(x * x) - f(y * y))], np.float32)


def tree_sum(values):
    """The Philox mode's fixed tree over per-sample values float32 (N, C), restated in numpy float32: sample s to sub-stream s mod S, each
    sub-stream added in increasing order from 0.0f, the sub-sums pairwise, the root / (float)N"""
    v = np.asarray(values, np.float32)
    n = len(v)
    S = 16 if n >= 16 else 4 if n >= 4 else 1
    part = np.zeros((S,) + v.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for s in range(n):
            part[s % S] = part[s % S] + v[s]
        step = 1
        while step < S:
            for k in range(0, S, 2 * step):
                part[k] = part[k] + part[k + step]
            step *= 2
        return part[0] / np.float32(n)


def finish(root, mode):
    """the output floats of a visibility point from its tree root / N (float32 (C,)): mode 0 as it is, mode 1 the coefficients * 4 pi and
    two zeros, mode 2 with the trailing 1"""
    root = np.asarray(root, np.float32)
    if mode == SH9:
        with np.errstate(all="ignore"):
            return np.concatenate([(root[:9] * np.float32(12.566371)).astype(np.float32), root[9:10], np.zeros(2, np.float32)])
    if mode == DISTANCE:
        return np.concatenate([root, np.ones(1, np.float32)])
    return root


def assert_same_bits(got, want, what):
    """every item and channel, NaN equal to NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        with np.errstate(all="ignore"):
            diff = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        rows = int((~same).reshape(len(same), -1).any(-1).sum()) if same.ndim > 1 else int((~same).sum())
        raise AssertionError(f"{what}: {rows} of {len(same)} rows differ (max abs diff {diff:.3e}); first at {i}: got {got[i]!r} want {want[i]!r}")
