"""The feature-buffer checker: tests/aov_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, plus the bitwise
comparison the feature-buffer tests share.  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

_lib = None


def shim():
    global _lib
    if _lib is None:
        lib = compile_checker("aov_oracle.c")
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.aov_frame.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
        lib.aov_frame.restype = ci
        lib.aov_accumulate.argtypes = [vp, vp, ctypes.c_size_t, ci]
        lib.aov_accumulate.restype = None
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def oracle_frame(rtx, params, spheres, tris, infos, frame, rect=None, accel=True):
    """(albedo, normal_depth) of one feature frame, each [h, w, 4] float32, for the pixel rectangle (x0, y0, x1, y1) of the image"""
    p = np.array(params, dtype=rtx.PARAMS).reshape(()).copy()
    s = np.ascontiguousarray(spheres, rtx.SPHERE)
    t = np.ascontiguousarray(tris, rtx.TRIANGLE)
    m = np.ascontiguousarray(infos, rtx.MESHINFO)
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, int(p["width"]), int(p["height"]))
    a, n = np.empty((y1 - y0, x1 - x0, 4), np.float32), np.empty((y1 - y0, x1 - x0, 4), np.float32)
    rc = shim().aov_frame(_p(p), _p(s), len(s), _p(t), len(t), _p(m), len(m), int(frame), x0, y0, x1, y1, 1 if accel else 0, _p(a), _p(n))
    assert rc == 0, f"aov_frame failed: {rc}"
    return a, n


def oracle_planes(rtx, params, spheres, tris, infos, frames, rect=None):
    """the two planes after accumulating the feature frames `frames` in order, starting from zeroed planes"""
    acc, k = None, 0
    for f in frames:
        cur = oracle_frame(rtx, params, spheres, tris, infos, f, rect)
        if acc is None:
            acc = [np.zeros_like(cur[0]), np.zeros_like(cur[1])]
        for a, c in zip(acc, cur):
            shim().aov_accumulate(_p(a), _p(c), a.size, k)
        k += 1
    return acc


def assert_same_bits(got, want, what):
    """every pixel and channel, NaN equal to NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same)
        y, x, c = bad[0]
        with np.errstate(all="ignore"):
            diff = float(np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        raise AssertionError(f"{what}: {int((~same).any(-1).sum())} of {same.shape[0] * same.shape[1]} pixels differ (max abs diff {diff:.3e}); "
                             f"first at (x {x}, y {y}, channel {c}): got {got[y, x, c]!r} want {want[y, x, c]!r}")
