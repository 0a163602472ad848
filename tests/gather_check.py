"""The gather-query checker: tests/gather_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, plus what the gather
tests share.  Test infrastructure only."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from radiance_check import assert_same_bits  # noqa: F401  (every float, NaN equal to NaN)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

COSINE, SH9 = 0, 1
_lib = None


def shim():
    global _lib
    if _lib is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
        so = os.path.join(tempfile.mkdtemp(prefix="gather_oracle_"), "libgth.so")
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(HERE, "gather_oracle.c"), "-lm"])
        lib = ctypes.CDLL(so)
        vp, ci, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        lib.gth_gather.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, u32, u32, ci, ci, vp, vp]
        lib.gth_sample.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, u32, u32, u32, ci, ci, vp]
        lib.gth_direction.argtypes = [vp, u32, u32, u32, ci, vp]
        for f in (lib.gth_gather, lib.gth_sample, lib.gth_direction):
            f.restype = ci
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scene(rtx, params, spheres, tris, infos):
    return (np.array(params, dtype=rtx.PARAMS).reshape(()).copy(), np.ascontiguousarray(spheres, rtx.SPHERE),
            np.ascontiguousarray(tris, rtx.TRIANGLE), np.ascontiguousarray(infos, rtx.MESHINFO))


def oracle_gather(rtx, params, spheres, tris, infos, points, samples, seed=0, first_index=0, mode=COSINE, accel=True, count_casts=False):
    """float32 (n, 4) in mode 0, (n, 9, 4) in mode 1: the gather query of every point on the CPU oracle (and the casts its samples made,
    if asked for)"""
    p, s, t, m = _scene(rtx, params, spheres, tris, infos)
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 9, 4) if mode == SH9 else (len(r), 4), np.float32)
    casts = ctypes.c_uint64(0)
    rc = shim().gth_gather(_p(p), _p(s), len(s), _p(t), len(t), _p(m), len(m), _p(r), len(r), int(samples), int(seed) & 0xFFFFFFFF,
                           int(first_index) & 0xFFFFFFFF, int(mode), 1 if accel else 0, _p(out),
                           ctypes.cast(ctypes.byref(casts), ctypes.c_void_p))
    assert rc == 0, f"gth_gather failed: {rc}"
    return (out, casts.value) if count_casts else out


def oracle_sample(rtx, params, spheres, tris, infos, point, sample, seed=0, index=0, mode=COSINE, accel=True):
    """float32 (3,): L of sample `sample` alone of one point with stream index `index`"""
    p, s, t, m = _scene(rtx, params, spheres, tris, infos)
    r = np.ascontiguousarray(point, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(3, np.float32)
    rc = shim().gth_sample(_p(p), _p(s), len(s), _p(t), len(t), _p(m), len(m), _p(r), int(sample), int(seed) & 0xFFFFFFFF,
                           int(index) & 0xFFFFFFFF, int(mode), 1 if accel else 0, _p(out))
    assert rc == 0, f"gth_sample failed: {rc}"
    return out


def direction(normal, sample, seed=0, index=0, mode=COSINE):
    """float32 (3,): the direction of sample `sample` of a point with that normal and stream index"""
    n = np.ascontiguousarray(normal, np.float32).reshape(3).copy()
    out = np.empty(3, np.float32)
    assert shim().gth_direction(_p(n), int(sample), int(seed) & 0xFFFFFFFF, int(index) & 0xFFFFFFFF, int(mode), _p(out)) == 0
    return out


def directions(rtx, points, sample, seed=0, first_index=0, mode=COSINE):
    """float32 (n, 3): sample `sample`'s direction of every point of a batch"""
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    return np.stack([direction(r["direction"][i], sample, seed, (first_index + i) & 0xFFFFFFFF, mode) for i in range(len(r))]) \
        if len(r) else np.zeros((0, 3), np.float32)


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


def surface_points(rtx, hits, t_max=np.inf, offset=1e-3):
    """The points the GPU tests gather at: hitPoint + offset * normal with the normal, misses kept with origin 0 and n = 0"""
    pts = np.zeros(len(hits), rtx.RAY)
    n = np.asarray(hits["normal"], np.float32)
    pts["origin"] = (np.asarray(hits["hitPoint"], np.float32) + np.float32(offset) * n).astype(np.float32)
    pts["direction"] = n
    pts["tMax"] = t_max
    return pts
