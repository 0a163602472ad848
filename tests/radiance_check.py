"""The radiance-query checker: tests/radiance_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, plus what the
radiance tests share.  Test infrastructure only."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_lib = None


def shim():
    global _lib
    if _lib is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
        so = os.path.join(tempfile.mkdtemp(prefix="radiance_oracle_"), "librad.so")
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(HERE, "radiance_oracle.c"), "-lm"])
        lib = ctypes.CDLL(so)
        vp, ci, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        lib.rad_trace.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, u32, u32, ci, vp, vp]
        lib.rad_sample.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, u32, u32, u32, ci, vp]
        lib.rad_camera_rays.argtypes = [vp, ci, vp]
        for f in (lib.rad_trace, lib.rad_sample, lib.rad_camera_rays):
            f.restype = ci
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _scene(rtx, params, spheres, tris, infos):
    return (np.array(params, dtype=rtx.PARAMS).reshape(()).copy(), np.ascontiguousarray(spheres, rtx.SPHERE),
            np.ascontiguousarray(tris, rtx.TRIANGLE), np.ascontiguousarray(infos, rtx.MESHINFO))


def oracle_radiance(rtx, params, spheres, tris, infos, rays, samples, seed=0, first_index=0, accel=True, count_casts=False):
    """float32 (n, 4): the radiance query of every ray on the CPU oracle (and the casts its samples made, if asked for)"""
    p, s, t, m = _scene(rtx, params, spheres, tris, infos)
    r = np.ascontiguousarray(rays, rtx.RAY).reshape(-1)
    out = np.empty((len(r), 4), np.float32)
    casts = ctypes.c_uint64(0)
    rc = shim().rad_trace(_p(p), _p(s), len(s), _p(t), len(t), _p(m), len(m), _p(r), len(r), int(samples), int(seed) & 0xFFFFFFFF,
                          int(first_index) & 0xFFFFFFFF, 1 if accel else 0, _p(out), ctypes.cast(ctypes.byref(casts), ctypes.c_void_p))
    assert rc == 0, f"rad_trace failed: {rc}"
    return (out, casts.value) if count_casts else out


def oracle_sample(rtx, params, spheres, tris, infos, ray, sample, seed=0, index=0, accel=True):
    """float32 (3,): sample `sample` alone of one ray with stream index `index`"""
    p, s, t, m = _scene(rtx, params, spheres, tris, infos)
    r = np.ascontiguousarray(ray, rtx.RAY).reshape(-1)[:1].copy()
    out = np.empty(3, np.float32)
    rc = shim().rad_sample(_p(p), _p(s), len(s), _p(t), len(t), _p(m), len(m), _p(r), int(sample), int(seed) & 0xFFFFFFFF,
                           int(index) & 0xFFFFFFFF, 1 if accel else 0, _p(out))
    assert rc == 0, f"rad_sample failed: {rc}"
    return out


def frame_camera_rays(rtx, params, frame):
    """RAY (width * height,): sample 0's camera ray of every pixel of frame `frame` as frag draws it in Philox mode, in pixelIndex order"""
    p = np.array(params, dtype=rtx.PARAMS).reshape(()).copy()
    rays = np.zeros(int(p["width"]) * int(p["height"]), rtx.RAY)
    assert shim().rad_camera_rays(_p(p), int(frame), _p(rays)) == 0
    return rays


def tree_sum(values):
    """The Philox mode's fixed tree over per-sample values float32 (N, 3), restated in numpy float32: sample s to sub-stream s mod S, each
    sub-stream added in increasing order from 0.0f, the sub-sums pairwise, the root / (float)N"""
    v = np.asarray(values, np.float32)
    n = len(v)
    S = 16 if n >= 16 else 4 if n >= 4 else 1
    part = np.zeros((S, 3), np.float32)
    for s in range(n):
        part[s % S] = part[s % S] + v[s]
    step = 1
    while step < S:
        for k in range(0, S, 2 * step):
            part[k] = part[k] + part[k + step]
        step *= 2
    return part[0] / np.float32(n)


def assert_same_bits(got, want, what):
    """every ray and channel, NaN equal to NaN"""
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
