"""The denoiser's checker: tests/denoise_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, a float64 numpy
restatement of the same definition written from the text of include/rt.h (exact 2**x), and the inputs the denoiser tests share.
Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

DEFAULTS = dict(iterations=5, demodulate=0, sigmaColour=16.0, sigmaNormal=1.0, sigmaDepth=0.5)      # RT_DENOISE_DEFAULT_* of include/rt.h
TIGHT = dict(sigmaColour=0.05, sigmaNormal=0.02, sigmaDepth=0.003)
WIDE = dict(sigmaColour=4.0, sigmaNormal=0.5, sigmaDepth=0.2)

_lib = None


def shim():
    global _lib
    if _lib is None:
        lib = compile_checker("denoise_oracle.c")
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.denoise_image.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, cf, cf, ci, vp]
        lib.denoise_image.restype = ci
        lib.denoise_exp2.argtypes = [cf]
        lib.denoise_exp2.restype = cf
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def checker(C, A, G, iterations=5, demodulate=0, sigmaColour=16.0, sigmaNormal=1.0, sigmaDepth=0.5, variant=0):
    """the denoised plane [H, W, 4] float32 of the C checker; variant 1 / 2 = the two deliberate misreadings (clamped borders, a colour
    sigma that does not halve)"""
    C, A, G = (np.ascontiguousarray(a, np.float32) for a in (C, A, G))
    assert C.shape == A.shape == G.shape and C.ndim == 3 and C.shape[2] == 4
    H, W = C.shape[:2]
    out = np.empty_like(C)
    rc = shim().denoise_image(_p(C), _p(A), _p(G), W, H, int(iterations), int(demodulate), sigmaColour, sigmaNormal, sigmaDepth, int(variant), _p(out))
    assert rc == 0
    return out


def twin64(C, A, G, iterations=5, demodulate=0, sigmaColour=16.0, sigmaNormal=1.0, sigmaDepth=0.5):
    """The definition in float64 with exact 2**x, written from the header's text: one vectorised shift per tap, taps outside the image
    skipped.  The sigmas are taken as the float32 values the checker receives."""
    C, A, G = (np.asarray(a, np.float32).astype(np.float64) for a in (C, A, G))
    H, W = C.shape[:2]
    sc, sn, sd = (float(np.float32(v)) for v in (sigmaColour, sigmaNormal, sigmaDepth))
    if demodulate:
        d = np.maximum(A[..., :3] + (1.0 - A[..., 3:4]), float(np.float32(0.01)))
    else:
        d = np.ones((H, W, 3))
    e = C[..., :3] / d
    kn, kz = 1.0 / (sn * sn), 1.0 / (sd * sd)
    zs = kz / (G[..., 3] ** 2 + float(np.float32(1e-6)))
    h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    for i in range(iterations):
        s = 1 << i
        kc = (1.0 / (sc * sc)) * 4.0 ** i
        sw = np.zeros((H, W))
        acc = np.zeros((H, W, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # pixels p = (y, x) whose tap q = (y + oy, x + ox) is inside
                y0, y1 = max(0, -oy), min(H, H - oy)
                x0, x1 = max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                dn2 = ((G[P][..., :3] - G[Q][..., :3]) ** 2).sum(-1)
                dz2 = (G[P][..., 3] - G[Q][..., 3]) ** 2
                dc2 = ((e[P] - e[Q]) ** 2).sum(-1)
                w = h[dy + 2] * h[dx + 2] * np.exp2(-(dn2 * kn + dz2 * zs[P] + dc2 * kc))
                sw[P] += w
                acc[P] += w[..., None] * e[Q]
        e = acc / sw[..., None]
    return np.concatenate([e * d, C[..., 3:4]], -1)


def random_inputs(W, H, seed, colour_max=1.0):
    """a random image and random guides of a plausible kind: colours in [0, colour_max], albedo and coverage in [0, 1], unit-ish normals
    in a few flat regions with noise, depths in [1, 20] (0 where the coverage is 0)"""
    rng = np.random.default_rng(seed)
    C = rng.uniform(0.0, colour_max, (H, W, 4)).astype(np.float32)
    A = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    A[..., 3] = np.round(A[..., 3] * 4) / 4
    region = (np.add.outer(np.arange(H) // 7, np.arange(W) // 9) % 3)
    normals = np.array([[0, 1, 0], [1, 0, 0], [0.6, 0.0, -0.8]], np.float32)[region]
    G = np.empty((H, W, 4), np.float32)
    G[..., :3] = normals + rng.normal(0, 0.02, (H, W, 3)).astype(np.float32)
    G[..., 3] = (1.0 + 19.0 * rng.uniform(0, 1, (H, W))).astype(np.float32) * (A[..., 3] > 0)
    return C, A, G


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]) ** 2)))
