"""The variance-guided denoiser's checker: tests/vdenoise_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, and a
float64 numpy restatement of the same definition written from the text of include/rt.h (exact 2**x).  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker
from denoise_check import random_inputs, rmse          # noqa: F401  (shared by the tests of both filters)

# RT_VDENOISE_DEFAULT_* of include/rt.h
DEFAULTS = dict(iterations=3, demodulate=1, sigmaLuminance=8.0, sigmaNormal=0.25, sigmaDepth=0.5)
TIGHT = dict(sigmaLuminance=0.5, sigmaNormal=0.02, sigmaDepth=0.003)
WIDE = dict(sigmaLuminance=8.0, sigmaNormal=0.5, sigmaDepth=0.2)

_lib = None


def shim():
    global _lib
    if _lib is None:
        lib = compile_checker("vdenoise_oracle.c")
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.vdenoise_image.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, cf, cf, ci, vp, vp]
        lib.vdenoise_variance.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, ci, vp]
        lib.vdenoise_pass.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, cf, ci, vp, vp]
        for f in (lib.vdenoise_image, lib.vdenoise_variance, lib.vdenoise_pass):
            f.restype = ci
        lib.vdenoise_exp2.argtypes = [cf]
        lib.vdenoise_exp2.restype = cf
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _planes(C, A, G):
    C, A, G = (np.ascontiguousarray(a, np.float32) for a in (C, A, G))
    assert C.shape == A.shape == G.shape and C.ndim == 3 and C.shape[2] == 4
    return C, A, G


def checker(C, A, G, iterations=5, demodulate=0, sigmaLuminance=4.0, sigmaNormal=1.0, sigmaDepth=0.5, variant=0):
    """(the denoised plane [H, W, 4], var_0 [H, W]) float32 of the C checker; variant 1 / 2 / 3 = the deliberate misreadings (clamped
    borders, the prefilter at spacing s, variance weighted by w)"""
    C, A, G = _planes(C, A, G)
    H, W = C.shape[:2]
    out, var = np.empty_like(C), np.empty((H, W), np.float32)
    rc = shim().vdenoise_image(_p(C), _p(A), _p(G), W, H, int(iterations), int(demodulate), sigmaLuminance, sigmaNormal, sigmaDepth,
                               int(variant), _p(out), _p(var))
    assert rc == 0
    return out, var


def checker_variance(C, A, G, demodulate=0, sigmaNormal=1.0, sigmaDepth=0.5, variant=0):
    C, A, G = _planes(C, A, G)
    H, W = C.shape[:2]
    var = np.empty((H, W), np.float32)
    assert shim().vdenoise_variance(_p(C), _p(A), _p(G), W, H, int(demodulate), sigmaNormal, sigmaDepth, int(variant), _p(var)) == 0
    return var


def checker_pass(e, var, G, step=1, sigmaLuminance=4.0, sigmaNormal=1.0, sigmaDepth=0.5, variant=0):
    """one pass from injected (e_i [H, W, 3], var_i [H, W]) -> (e_{i+1}, var_{i+1})"""
    e, var, G = (np.ascontiguousarray(a, np.float32) for a in (e, var, G))
    H, W = var.shape
    assert e.shape == (H, W, 3) and G.shape == (H, W, 4)
    e2, var2 = np.empty_like(e), np.empty_like(var)
    assert shim().vdenoise_pass(_p(e), _p(var), _p(G), W, H, int(step), sigmaLuminance, sigmaNormal, sigmaDepth, int(variant), _p(e2), _p(var2)) == 0
    return e2, var2


def _lum64(e):
    c = [float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722)]
    return c[0] * e[..., 0] + c[1] * e[..., 1] + c[2] * e[..., 2]


def _taps(H, W, radius, spacing):
    """(dy, dx, P, Q): for each tap of the square window the slices of the pixels p whose tap q lies inside, and of those taps"""
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            oy, ox = dy * spacing, dx * spacing
            y0, y1 = max(0, -oy), min(H, H - oy)
            x0, x1 = max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            yield dy, dx, (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def twin64(C, A, G, iterations=5, demodulate=0, sigmaLuminance=4.0, sigmaNormal=1.0, sigmaDepth=0.5):
    """The definition in float64 with exact 2**x, written from the header's text: one vectorised shift per tap, taps outside the image
    skipped.  The sigmas are taken as the float32 values the checker receives.  Returns (the denoised plane, var_0)."""
    C, A, G = (np.asarray(a, np.float32).astype(np.float64) for a in (C, A, G))
    H, W = C.shape[:2]
    sl, sn, sd = (float(np.float32(v)) for v in (sigmaLuminance, sigmaNormal, sigmaDepth))
    eps = float(np.float32(1e-6))
    if demodulate:
        d = np.maximum(A[..., :3] + (1.0 - A[..., 3:4]), float(np.float32(0.01)))
    else:
        d = np.ones((H, W, 3))
    e = C[..., :3] / d
    kn, kz = 1.0 / (sn * sn), 1.0 / (sd * sd)
    zs = kz / (G[..., 3] ** 2 + eps)

    def geometry(P, Q):
        dn2 = ((G[P][..., :3] - G[Q][..., :3]) ** 2).sum(-1)
        dz2 = (G[P][..., 3] - G[Q][..., 3]) ** 2
        return dn2 * kn + dz2 * zs[P]

    # estimate
    lum = _lum64(e)
    sg, m1, m2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for _, _, P, Q in _taps(H, W, 3, 1):
        g = np.exp2(-geometry(P, Q))
        sg[P] += g
        m1[P] += g * lum[Q]
        m2[P] += g * lum[Q] ** 2
    mu = m1 / sg
    var = np.maximum(m2 / sg - mu * mu, 0.0)
    var0 = var.copy()
    h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    k3 = np.array([1 / 4, 1 / 2, 1 / 4])
    for i in range(iterations):
        pn, pd = np.zeros((H, W)), np.zeros((H, W))
        for dy, dx, P, Q in _taps(H, W, 1, 1):
            pn[P] += k3[dy + 1] * k3[dx + 1] * var[Q]
            pd[P] += k3[dy + 1] * k3[dx + 1]
        kl = 1.0 / (sl * np.sqrt(pn / pd) + eps)
        lum = _lum64(e)
        sw, sv, acc = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
        for dy, dx, P, Q in _taps(H, W, 2, 1 << i):
            w = h[dy + 2] * h[dx + 2] * np.exp2(-(geometry(P, Q) + np.abs(lum[P] - lum[Q]) * kl[P]))
            sw[P] += w
            acc[P] += w[..., None] * e[Q]
            sv[P] += w * w * var[Q]
        e = acc / sw[..., None]
        var = sv / (sw * sw)
    return np.concatenate([e * d, C[..., 3:4]], -1), var0
