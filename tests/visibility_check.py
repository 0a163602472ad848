"""The visibility-gather checker: tests/visibility_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, plus what the
visibility tests share.  Test infrastructure only."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from gather_check import assert_same_bits, surface_points, tree_sum  # noqa: F401  (shared with the gather tests)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

COSINE, SH9, DISTANCE = 0, 1, 2
MODES = (COSINE, SH9, DISTANCE)
CHANNELS = {COSINE: 4, SH9: 10, DISTANCE: 3}
_lib = None


def shim():
    global _lib
    if _lib is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
        so = os.path.join(tempfile.mkdtemp(prefix="visibility_oracle_"), "libvis.so")
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(HERE, "visibility_oracle.c"), "-lm"])
        lib = ctypes.CDLL(so)
        vp, ci, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        lib.vis_gather.argtypes = [vp, ci, vp, ci, vp, ci, ci, vp, ci, ci, u32, u32, ci, ci, vp]
        lib.vis_sample.argtypes = [vp, ci, vp, ci, vp, ci, ci, vp, u32, u32, u32, ci, ci, vp]
        lib.vis_direction.argtypes = [vp, u32, u32, u32, ci, vp]
        for f in (lib.vis_gather, lib.vis_sample, lib.vis_direction):
            f.restype = ci
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scene(rtx, spheres, tris, infos):
    return (np.ascontiguousarray(spheres, rtx.SPHERE), np.ascontiguousarray(tris, rtx.TRIANGLE), np.ascontiguousarray(infos, rtx.MESHINFO))


def oracle_visibility(rtx, spheres, tris, infos, points, samples, seed=0, first_index=0, mode=COSINE, intersect=0, accel=True):
    """float32 (n, 4) in modes 0 and 2, (n, 12) in mode 1: the visibility gather of every point on the CPU oracle"""
    s, t, m = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(points, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 12 if mode == SH9 else 4), np.float32)
    rc = shim().vis_gather(_p(s), len(s), _p(t), len(t), _p(m), len(m), int(intersect), _p(r), len(r), int(samples), int(seed) & 0xFFFFFFFF,
                           int(first_index) & 0xFFFFFFFF, int(mode), 1 if accel else 0, _p(out))
    assert rc == 0, f"vis_gather failed: {rc}"
    return out


def oracle_sample(rtx, spheres, tris, infos, point, sample, seed=0, index=0, mode=COSINE, intersect=0, accel=True):
    """float32 (4,), (10,) or (3,): the channels of sample `sample` alone of one (traced) point with stream index `index` — mode 0
    (v ? d : 0, v), mode 1 (v ? Y_k : 0, v), mode 2 (r, r * r, hit)"""
    s, t, m = _scene(rtx, spheres, tris, infos)
    r = np.ascontiguousarray(point, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(10, np.float32)
    rc = shim().vis_sample(_p(s), len(s), _p(t), len(t), _p(m), len(m), int(intersect), _p(r), int(sample), int(seed) & 0xFFFFFFFF,
                           int(index) & 0xFFFFFFFF, int(mode), 1 if accel else 0, _p(out))
    assert rc == CHANNELS[mode], f"vis_sample failed: {rc}"
    return out[:rc].copy()


def direction(normal, sample, seed=0, index=0, mode=COSINE):
    """float32 (3,): the direction of sample `sample` of a point with that normal and stream index"""
    n = np.ascontiguousarray(normal, np.float32).reshape(3).copy()
    out = np.empty(3, np.float32)
    assert shim().vis_direction(_p(n), int(sample), int(seed) & 0xFFFFFFFF, int(index) & 0xFFFFFFFF, int(mode), _p(out)) == 0
    return out


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


def finish(root, mode):
    """the output floats of a point from its tree root / N (float32 (C,)): mode 0 as it is, mode 1 the coefficients * 4 pi and two zeros,
    mode 2 with the trailing 1"""
    root = np.asarray(root, np.float32)
    if mode == SH9:
        with np.errstate(all="ignore"):
            return np.concatenate([(root[:9] * np.float32(12.566371)).astype(np.float32), root[9:10], np.zeros(2, np.float32)])
    if mode == DISTANCE:
        return np.concatenate([root, np.ones(1, np.float32)])
    return root
