"""Which refusal an image-filter entry reports, and with which code and text: a fixed walk over rt_denoise, rt_temporal,
rt_denoise_temporal, rt_denoise_variance, their readers, info getters and resets, and the rt_multi_ forms, through every state in which
they refuse — before rt_set_params, before a render, without a feature frame, without a temporal call (and without both: the context
entries look at the feature planes first, the handle's at the temporal image first), a temporal image of another size, rows of the
image, one out-of-range value per parameter field, a null destination, wrong sizes, a null info pointer, a null handle.  The C entries
are called directly, so the code and rt_last_error / rt_multi_last_error come back verbatim.  Every call in the walk is refused before
it reaches the device; the frames that set the states up are 70 x 45 and 48 x 30.

walk(rtx) -> [(label, return code, message)]; tests/golden/image_filter_refusals.json is that list as the library BEFORE the filters'
host code was folded into one path gave it (tests/test_gpu_image_filter_refusals.py compares).  As a script: prints the list as JSON.
"""
import ctypes
import json
import os
import sys

import numpy as np

W, H, W2, H2 = 70, 45, 48, 30


def walk(rtx):
    lib = rtx.load_library()
    out = []
    big = np.zeros(W * H * 4 + 8, np.float32)           # a destination large enough for every size the walk names
    fp = big.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    vp = big.ctypes.data_as(ctypes.c_void_p)
    info = np.zeros(8, np.float64)
    ip = info.ctypes.data_as(ctypes.c_void_p)

    def buffers(w, h):
        mgr = rtx.scenes.mesh_test_scene(w, h)
        mgr.numRaysPerPixel = 2
        return mgr.build_buffers()

    def record(owner, state, last_error, handle, name, *args, note=""):
        rc = getattr(lib, name)(handle, *args)
        msg = (last_error(handle) or b"").decode() if rc != 0 and handle is not None else ""
        out.append((f"{owner} | {state} | {name}{' ' + note if note else ''}", int(rc), msg))

    def record_of(owner, state, last_error, handle):
        return lambda name, *args, note="": record(owner, state, last_error, handle, name, *args, note=note)

    def params_of(dtype, defaults, **fields):
        p = np.zeros((), dtype)
        for k, v in defaults.items():
            p[k] = v
        for k, v in fields.items():
            if k.startswith("reserved"):
                p["_reserved"][int(k[-1])] = v
            else:
                p[k] = v
        return p

    def dn(**f):
        return params_of(rtx.DENOISE_PARAMS, rtx.DENOISE_DEFAULTS, **f)

    def tm(**f):
        return params_of(rtx.TEMPORAL_PARAMS, rtx.TEMPORAL_DEFAULTS, **f)

    def vd(**f):
        return params_of(rtx.VDENOISE_PARAMS, rtx.VDENOISE_DEFAULTS, **f)

    def ptr(p):
        return p.ctypes.data_as(ctypes.c_void_p)

    def fmt(fields):
        return ",".join(f"{k}={v}" for k, v in fields.items())

    SOURCE1 = vd(source=1)
    BAD_DENOISE = [dict(iterations=0), dict(iterations=7), dict(demodulate=2), dict(sigmaColour=0.0), dict(sigmaNormal=-1.0),
                   dict(sigmaDepth=float("nan")), dict(iterations=0, demodulate=2), dict(demodulate=-1, sigmaColour=float("inf"))]
    BAD_TEMPORAL = [dict(maxHistory=0), dict(maxHistory=4097), dict(depthTolerance=0.0), dict(normalTolerance=float("inf")),
                    dict(maxHistory=-1, depthTolerance=float("nan"))]
    BAD_VDENOISE = [dict(iterations=0), dict(iterations=7), dict(demodulate=2), dict(source=2), dict(source=-1), dict(sigmaLuminance=0.0),
                    dict(sigmaNormal=-1.0), dict(sigmaDepth=float("nan")), dict(reserved0=1), dict(reserved1=1),
                    dict(iterations=0, demodulate=2), dict(demodulate=2, source=2), dict(source=2, sigmaNormal=0.0),
                    dict(sigmaDepth=0.0, reserved0=1)]

    # ---- the two owners' entries under one set of names --------------------------------------------------------------------------
    CTX = dict(prefix="rt_", filters=("rt_denoise", "rt_temporal", "rt_denoise_temporal", "rt_denoise_variance"),
               # (entry, floats per pixel, takes a float pointer)
               planes=(("rt_read_denoised", 4, True), ("rt_copy_denoised_to_device", 4, False), ("rt_read_temporal", 4, True),
                       ("rt_copy_temporal_to_device", 4, False), ("rt_read_temporal_history", 1, True), ("rt_read_variance", 1, True),
                       ("rt_copy_variance_to_device", 1, False)),
               displays=("rt_read_denoised_display", "rt_read_temporal_display"),
               infos=("rt_get_denoise_info", "rt_get_temporal_info", "rt_get_vdenoise_info", "rt_get_aov_info"),
               resets=("rt_reset_temporal",))
    MULTI = dict(prefix="rt_multi_", filters=("rt_multi_denoise", "rt_multi_temporal", "rt_multi_denoise_temporal", "rt_multi_denoise_variance"),
                 planes=(("rt_multi_read_denoised", 4, True), ("rt_multi_read_temporal", 4, True), ("rt_multi_read_temporal_history", 1, True),
                         ("rt_multi_read_variance", 1, True)),
                 displays=("rt_multi_read_denoised_display", "rt_multi_read_temporal_display", "rt_multi_read_display"),
                 infos=(), resets=("rt_multi_reset_temporal",))

    def filters(rec, E, note=""):
        """the four filter calls with their defaults, the variance filter also with source 1"""
        for name in E["filters"]:
            rec(name, None, note=note)
        rec(E["filters"][3], ptr(SOURCE1), note=("source=1 " + note).strip())

    def bad_parameters(rec, E, note=""):
        d, t, dt, v = E["filters"]
        for f in BAD_DENOISE:
            rec(d, ptr(dn(**f)), note=(fmt(f) + " " + note).strip())
            rec(dt, ptr(dn(**f)), note=(fmt(f) + " " + note).strip())
        for f in BAD_TEMPORAL:
            rec(t, ptr(tm(**f)), note=(fmt(f) + " " + note).strip())
        for f in BAD_VDENOISE:
            rec(v, ptr(vd(**f)), note=(fmt(f) + " " + note).strip())

    def readers(rec, E, w, h, sizes, skip=()):
        """every reader (but `skip`) with a destination and each of `sizes` (names of counts for a w x h image), then with a null destination"""
        px = w * h
        counts = {"exact": None, "one less": -1, "one more": 1, "float4 size": px * 4, "one-float size": px, "zero": 0}
        for name, per, floats in E["planes"]:
            n = px * per
            for s in sizes:
                k = n if s == "exact" else n + counts[s] if s in ("one less", "one more") else counts[s]
                if k == n and s != "exact":
                    continue
                rec(name, fp if floats else vp, k, note=s)
            rec(name, None, n, note="null destination")
            rec(name, None, n + 1, note="null destination, one more")
        for name in E["displays"]:
            if name in skip:
                continue
            for s in sizes:
                k = px if s == "exact" else px + counts[s] if s in ("one less", "one more") else counts[s]
                if k == px and s != "exact":
                    continue
                rec(name, vp, k, note=s)
            rec(name, None, px, note="null destination")
            rec(name, None, px + 1, note="null destination, one more")

    def null_handle(E, owner):
        rec = record_of(owner, "null handle", None, None)
        for name in E["filters"]:
            rec(name, None)
        for name, per, floats in E["planes"]:
            rec(name, fp if floats else vp, 0)
        for name in E["displays"]:
            rec(name, vp, 0)
        for name in E["infos"]:
            rec(name, ip)
        for name in E["resets"]:
            rec(name)

    WRONG = ("one less", "one more", "float4 size", "one-float size", "zero")
    big_params, spheres, tris, infos = buffers(W, H)
    small_params = buffers(W2, H2)[0]

    # ---- a context ---------------------------------------------------------------------------------------------------------------
    null_handle(CTX, "context")
    with rtx.Tracer(0) as t:
        def at(state):
            return record_of("context", state, lib.rt_last_error, t._ctx)
        rec = at("before rt_set_params")
        filters(rec, CTX)
        bad_parameters(rec, CTX)
        readers(rec, CTX, W, H, ("exact",))
        for name in CTX["infos"]:
            rec(name, None, note="null info")

        t.set_params(big_params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        filters(at("before any render"), CTX)
        readers(at("before any render"), CTX, W, H, ("exact",))
        t.render(0, 1)
        filters(at("rendered, no feature frame"), CTX)
        t.render_aov(0, 1)
        rec = at("feature frame, no temporal call")
        rec("rt_denoise_temporal", None)
        rec("rt_denoise_variance", ptr(SOURCE1), note="source=1")
        rec("rt_denoise_temporal", ptr(dn(iterations=9)), note="iterations=9")
        rec("rt_denoise_variance", ptr(vd(source=1, sigmaDepth=0.0)), note="source=1,sigmaDepth=0.0")
        readers(rec, CTX, W, H, ("exact",))

        t.temporal()
        t.denoise(iterations=1)
        t.denoise_variance(iterations=1)
        rec = at("every plane filled")
        bad_parameters(rec, CTX)
        readers(rec, CTX, W, H, WRONG)
        for name in CTX["infos"]:
            rec(name, None, note="null info")
        rec = at("after rt_reset_temporal")
        t.reset_temporal()
        rec("rt_denoise_temporal", None)
        rec("rt_denoise_variance", ptr(SOURCE1), note="source=1")
        for name, per, floats in CTX["planes"][2:5]:
            rec(name, fp if floats else vp, W * H * per, note="exact")
        rec("rt_read_temporal_display", vp, W * H, note="exact")
        t.temporal()

        # a temporal image of another size than the context's
        t.set_params(small_params)
        t.render(0, 1)
        rec = at("temporal image 70 x 45, image 48 x 30, no feature frame at 48 x 30")
        rec("rt_denoise_temporal", None)
        rec("rt_denoise_variance", ptr(SOURCE1), note="source=1")
        t.render_aov(0, 1)
        rec = at("temporal image 70 x 45, image 48 x 30")
        rec("rt_denoise_temporal", None)
        rec("rt_denoise_variance", ptr(SOURCE1), note="source=1")
        rec("rt_denoise_temporal", ptr(dn(demodulate=2)), note="demodulate=2")
        rec("rt_read_temporal", fp, W2 * H2 * 4, note="the image's size")
        rec("rt_read_temporal_history", fp, W2 * H2, note="the image's size")
        rec("rt_read_temporal_display", vp, W2 * H2, note="the image's size")
        rec("rt_read_denoised", fp, W2 * H2 * 4, note="the image's size")
        rec("rt_read_variance", fp, W2 * H2, note="the image's size")

        # rows of the image
        t.set_params(big_params)
        t.render(0, 1)
        t.render_aov(0, 1)
        t.set_rows(8, 16)
        rec = at("rt_set_rows(8, 16)")
        filters(rec, CTX)
        rec("rt_denoise", ptr(dn(iterations=0)), note="iterations=0")
        rec("rt_temporal", ptr(tm(maxHistory=0)), note="maxHistory=0")
        rec("rt_denoise_variance", ptr(vd(source=2)), note="source=2")
        t.set_bands(0, 2)
        filters(at("rt_set_bands(0, 2)"), CTX)
    with rtx.Tracer(0) as t:
        t.set_params(big_params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        t.set_bands(0, 2)
        t.render(0, 1)
        t.render_aov(0, 1)
        filters(record_of("context", "rt_set_bands(0, 2), rendered with a feature frame", lib.rt_last_error, t._ctx), CTX)

    # ---- a handle over two contexts of one device --------------------------------------------------------------------------------
    null_handle(MULTI, "handle")
    with rtx.MultiTracer([0, 0]) as m:
        def at(state):
            return record_of("handle", state, lib.rt_multi_last_error, m._m)
        rec = at("before rt_multi_set_params")
        filters(rec, MULTI)
        bad_parameters(rec, MULTI)
        readers(rec, MULTI, W, H, ("exact",))

        m.set_params(big_params)
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        filters(at("before any render"), MULTI)
        readers(at("before any render"), MULTI, W, H, ("exact",))
        m.render(0, 1)
        filters(at("rendered, no feature frame"), MULTI)
        m.render_aov(0, 1)
        rec = at("feature frame, no temporal call")
        rec("rt_multi_denoise_temporal", None)
        rec("rt_multi_denoise_variance", ptr(SOURCE1), note="source=1")
        rec("rt_multi_denoise_temporal", ptr(dn(iterations=9)), note="iterations=9")
        rec("rt_multi_denoise_variance", ptr(vd(source=1, sigmaDepth=0.0)), note="source=1,sigmaDepth=0.0")
        readers(rec, MULTI, W, H, ("exact",), skip=("rt_multi_read_display",))      # (the image exists: that read would succeed)

        m.temporal()
        m.denoise(iterations=1)
        m.denoise_variance(iterations=1)
        rec = at("every plane filled")
        bad_parameters(rec, MULTI)
        readers(rec, MULTI, W, H, WRONG)
        rec = at("after rt_multi_reset_temporal")
        m.reset_temporal()
        rec("rt_multi_denoise_temporal", None)
        rec("rt_multi_denoise_variance", ptr(SOURCE1), note="source=1")
        rec("rt_multi_read_temporal", fp, W * H * 4, note="exact")
        rec("rt_multi_read_temporal_history", fp, W * H, note="exact")
        rec("rt_multi_read_temporal_display", vp, W * H, note="exact")
        m.temporal()

        m.set_params(small_params)
        m.render(0, 1)
        rec = at("temporal image 70 x 45, image 48 x 30, no feature frame at 48 x 30")
        filters(rec, MULTI)
        m.render_aov(0, 1)
        rec = at("temporal image 70 x 45, image 48 x 30")
        rec("rt_multi_denoise_temporal", None)
        rec("rt_multi_denoise_variance", ptr(SOURCE1), note="source=1")
        rec("rt_multi_denoise_temporal", ptr(dn(demodulate=2)), note="demodulate=2")
        rec("rt_multi_read_temporal", fp, W2 * H2 * 4, note="the image's size")
        rec("rt_multi_read_temporal_history", fp, W2 * H2, note="the image's size")
        rec("rt_multi_read_temporal_display", vp, W2 * H2, note="the image's size")
        rec("rt_multi_read_denoised", fp, W2 * H2 * 4, note="the image's size")
        rec("rt_multi_read_denoised_display", vp, W2 * H2, note="the image's size")
        rec("rt_multi_read_variance", fp, W2 * H2, note="the image's size")
    with rtx.MultiTracer([0, 0]) as m:
        m.set_params(big_params)
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        m.render_aov(0, 1)
        filters(record_of("handle", "feature frame, nothing rendered", lib.rt_multi_last_error, m._m), MULTI)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import rtx_pkg
    print("[\n" + ",\n".join(json.dumps(list(e)) for e in walk(rtx_pkg.load())) + "\n]")
