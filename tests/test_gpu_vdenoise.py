"""The variance-guided denoiser on the GPU (rt_denoise_variance and rt_multi_denoise_variance): the denoised plane and var_0 bitwise
against tests/vdenoise_oracle.c, which is fed what rt_read_accum or rt_read_temporal, and rt_read_aov, return from the same context —
rendered and injected colours, ragged and degenerate image sizes (one column and one row past a 64 x 4 workgroup, an image smaller than
both windows), every iteration count that takes another path, both demodulation settings, both sources, the defaults and a tight sigma
set — and around it: the context's state untouched, the denoised plane shared with rt_denoise, the display step, every refusal, a
caller's stream, several contexts behind one handle."""
import ctypes

import numpy as np
import pytest

import denoise_check
import temporal_check
import vdenoise_check
from aov_check import assert_same_bits
from test_gpu_aov import hip_runtime
from test_gpu_denoise import assert_same_state, buffers_of, inject, loaded, state_of
from test_gpu_temporal import scene, show
from vdenoise_check import DEFAULTS, TIGHT, WIDE

pytestmark = pytest.mark.gpu

# 70 x 45: ragged tiles in both axes; 200 x 120: several workgroups; 9 x 7: the late passes' off-centre taps lie outside; 3 x 2: smaller
# than the 7 x 7 and the 5 x 5 window; one column; one row; 65 x 5: one column and one row past a 64 x 4 workgroup
SIZES = [(70, 45), (200, 120), (9, 7), (3, 2), (1, 40), (40, 1), (65, 5)]
DEFAULT_SIGMAS = {k: DEFAULTS[k] for k in ("sigmaLuminance", "sigmaNormal", "sigmaDepth")}
# (iterations, demodulate, source, sigmas)
SETTINGS = [(1, 1, 0, DEFAULT_SIGMAS), (2, 0, 1, TIGHT), (5, 1, 1, DEFAULT_SIGMAS), (5, 0, 0, TIGHT), (6, 1, 0, TIGHT), (6, 0, 1, WIDE)]


def prepared(rtx, name, w, h):
    """a context with one image frame, two feature frames and one rt_temporal call"""
    t = loaded(rtx, buffers_of(rtx, name, w, h))
    t.render(0, 1)
    t.render_aov(0, 2)
    t.temporal()
    return t


def want_of(t, source=0, **kw):
    C = t.read_temporal() if source else t.read_accum()
    return vdenoise_check.checker(C, t.read_aov(0), t.read_aov(1), **kw)


def assert_matches_checker(t, what, source=0, **kw):
    want, want_var = want_of(t, source, **kw)
    assert_same_bits(t.read_denoised(), want, f"{what}: the denoised plane")
    assert_same_bits(t.read_variance()[..., None], want_var[..., None], f"{what}: var_0")


def run_settings(t, what, settings):
    for colour in ("rendered", "injected"):
        if colour == "injected":
            inject(t, 7)
            t.temporal()                # (T blends the injected image into the rendered one)
        for iterations, demod, source, sig in settings:
            kw = dict(iterations=iterations, demodulate=demod, **sig)
            t.denoise_variance(source=source, **kw)
            assert_matches_checker(t, f"{what} {colour} source {source} {kw}", source, **kw)
            info = t.vdenoise_info()
            H, W = t._image_shape()
            assert (info["iterations"], info["source"], info["width"], info["height"]) == (iterations, source, W, H)
            assert info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"]


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_bitwise_against_the_checker(rtx, w, h):
    """mesh_test_scene's guides (silhouettes, sky, a checker floor, invisible lights); the rendered image, then injected colours up to 1e4"""
    with prepared(rtx, "mesh_test_scene", w, h) as t:
        run_settings(t, f"{w}x{h}", SETTINGS)


def test_sphere_in_view_bitwise_against_the_checker(rtx):
    with prepared(rtx, "sphere_in_view", 45, 45) as t:
        A = t.read_aov(0)
        assert ((A[..., 3] > 0) & (A[..., 3] < 1)).any() and (A[..., 3] == 0).any()          # a silhouette and sky
        run_settings(t, "sphere 45", SETTINGS[:4])


def test_defaults_are_the_headers(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        t.denoise_variance()
        got, var = t.read_denoised(), t.read_variance()
        assert_matches_checker(t, "null params", 0, **DEFAULTS)
        t.denoise_variance(**DEFAULTS)
        assert_same_bits(t.read_denoised(), got, "the defaults spelled out")
        assert_same_bits(t.read_variance()[..., None], var[..., None], "the defaults spelled out: var_0")
        info = t.vdenoise_info()
        assert (info["iterations"], info["source"]) == (DEFAULTS["iterations"], 0)


def test_non_finite_colours_return_and_give_the_checkers_bits(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        C = t.read_accum()
        C[::5, ::7, 0], C[1::5, ::7, 1], C[2::5, ::7, 2] = np.nan, np.inf, -np.inf
        t.write_accum(C, 1)
        for demod in (0, 1):
            kw = dict(iterations=3, demodulate=demod, **DEFAULT_SIGMAS)
            t.denoise_variance(**kw)
            assert_matches_checker(t, f"non-finite colours, demodulate {demod}", 0, **kw)
        assert np.isnan(t.read_denoised()).any()


def test_source_1_after_a_camera_step(rtx):
    """the temporal tests' sideways pose pair: T carries reprojected history, and the filter reads T, not the image"""
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    params = buffers[0]
    moved = temporal_check.posed(rtx, mgr, params, (0.25, 0.0, 0.0), 0.0)
    with loaded(rtx, buffers) as t:
        for k, p in enumerate((params, moved)):
            show(t, p, k)
            t.temporal()
        assert (t.read_temporal_history() > 1).mean() > 0.3                                  # (history was carried)
        assert (t.read_temporal() != t.read_accum()).any()
        for kw in (dict(DEFAULTS), dict(iterations=3, demodulate=1, **TIGHT)):
            t.denoise_variance(source=1, **kw)
            assert_matches_checker(t, f"after a camera step {kw}", 1, **kw)


def full_state(t):
    s = state_of(t)
    s.update(T=t.read_temporal(), N=t.read_temporal_history()[..., None], denoise_info=t.denoise_info(), temporal_info=t.temporal_info())
    return s


def assert_same_full_state(a, b, what):
    assert_same_state(a, b, what)
    for k in ("T", "N"):
        assert_same_bits(a[k], b[k], f"{what}: {k}")
    assert a["denoise_info"] == b["denoise_info"] and a["temporal_info"] == b["temporal_info"], what


def test_the_call_moves_no_other_state(rtx):
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as t, loaded(rtx, buffers) as plain:
        for c in (t, plain):
            c.render(0, 2)
            c.render_aov(0, 1)
        t.temporal()
        t.denoise(iterations=3)
        plain.denoise(iterations=3)
        before = full_state(t)
        for source in (0, 1):
            t.denoise_variance(iterations=3, source=source)
            assert_same_full_state(full_state(t), before, f"after rt_denoise_variance, source {source}")
            assert_matches_checker(t, f"source {source}", source, **dict(DEFAULTS, iterations=3))
        # the shared denoised plane carries nothing over: rt_denoise afterwards gives rt_denoise's bits
        t.denoise(iterations=3)
        assert_same_bits(t.read_denoised(), plain.read_denoised(), "rt_denoise after rt_denoise_variance")
        # a frame rendered afterwards equals the same frame without the call
        t.render(2, 1)
        plain.render(2, 1)
        assert_same_bits(t.read_accum(), plain.read_accum(), "frame 2 after the call")
        # interleaved with queued frames: the call settles the queue first, and the queue goes on after it
        for c in (t, plain):
            c.submit_frame(3)
            c.submit_frame(4)
        t.denoise_variance(iterations=2)
        assert_matches_checker(t, "after two queued frames", 0, **dict(DEFAULTS, iterations=2))
        for c in (t, plain):
            c.submit_frame(5)
            c.wait()
        assert_same_bits(t.read_accum(), plain.read_accum(), "queued frames around the call")
        assert t.stats()["numRenderedFrames"] == plain.stats()["numRenderedFrames"] == 6


def test_a_read_after_only_this_call_succeeds_and_a_size_change_recreates_the_planes(rtx):
    small = buffers_of(rtx, "mesh_test_scene", 48, 30)
    with loaded(rtx, buffers_of(rtx, "mesh_test_scene", 70, 45)) as t:
        t.render(0, 1)
        t.render_aov(0, 1)
        t.denoise_variance(iterations=2)                    # (no rt_denoise before it)
        assert t.read_denoised().shape == (45, 70, 4) and t.read_variance().shape == (45, 70)
        assert_matches_checker(t, "70x45", 0, **dict(DEFAULTS, iterations=2))
        assert t.denoise_info()["iterations"] == 0          # rt_denoise_info is rt_denoise's alone
        t.set_params(small[0])
        t.render(0, 1)
        t.render_aov(0, 1)
        t.denoise_variance(iterations=2)
        assert t.read_denoised().shape == (30, 48, 4) and t.read_variance().shape == (30, 48)
        assert_matches_checker(t, "48x30 after 70x45", 0, **dict(DEFAULTS, iterations=2))
        info = t.vdenoise_info()
        assert (info["width"], info["height"]) == (48, 30) and info["totalKernelMs"] == info["lastKernelMs"]
        t.denoise(iterations=2)
        want = denoise_check.checker(t.read_accum(), t.read_aov(0), t.read_aov(1), **dict(denoise_check.DEFAULTS, iterations=2))
        assert_same_bits(t.read_denoised(), want, "rt_denoise at the new size")


def test_a_callers_stream_gives_the_same_bits(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        t.denoise_variance(iterations=4)
        own, own_var = t.read_denoised(), t.read_variance()
        hip, stream = hip_runtime(), ctypes.c_void_p()
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        try:
            t.set_stream(stream.value)
            t.denoise_variance(iterations=4)
            got, got_var = t.read_denoised(), t.read_variance()
            t.set_stream(0)
        finally:
            hip.hipStreamDestroy(stream)
        assert_same_bits(got, own, "on a caller's stream")
        assert_same_bits(got_var[..., None], own_var[..., None], "var_0 on a caller's stream")


def test_copy_to_device_and_display(rtx):
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with prepared(rtx, "mesh_test_scene", 70, 45) as t, loaded(rtx, buffers) as second:
        t.denoise_variance()
        var = t.read_variance()
        hip, dev, back = hip_runtime(), ctypes.c_void_p(), np.zeros_like(var)
        assert hip.hipMalloc(ctypes.byref(dev), var.nbytes) == 0
        try:
            t.copy_variance_to_device(dev.value, var.size)
            assert hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), dev, var.nbytes, 2) == 0         # device to host
        finally:
            hip.hipFree(dev)
        assert_same_bits(back[..., None], var[..., None], "rt_copy_variance_to_device")
        assert (var > 0).any()
        # the display step of the denoised plane
        second.write_accum(t.read_denoised(), 1)
        np.testing.assert_array_equal(t.read_denoised_display(), second.read_display())
        assert t.read_denoised_display()[..., :3].any()


def _expect_refusal(rtx, call, match):
    with pytest.raises(rtx.RtError, match=match) as e:
        call()
    assert "(-2)" in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was(rtx):
    lib = rtx.load_library()
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with rtx.Tracer(0) as bare:
        _expect_refusal(rtx, lambda: bare.denoise_variance(), "rt_set_params")
    with loaded(rtx, buffers) as t:
        t.render(0, 1)
        _expect_refusal(rtx, lambda: t.denoise_variance(), "no feature frame")
        _expect_refusal(rtx, lambda: t.read_variance(), "rt_denoise_variance has not been called")
        t.render_aov(0, 1)
        _expect_refusal(rtx, lambda: t.denoise_variance(source=1), "rt_temporal has not been called")
        _expect_refusal(rtx, lambda: t.read_variance(), "rt_denoise_variance has not been called")
        _expect_refusal(rtx, lambda: t.read_denoised(), "rt_denoise has not been called")
        t.temporal()
        t.denoise_variance(iterations=2)
        plane, var, info, before = t.read_denoised(), t.read_variance(), t.vdenoise_info(), full_state(t)
        bad = [dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(demodulate=2), dict(source=2), dict(source=-1),
               dict(sigmaLuminance=0.0), dict(sigmaNormal=-1.0), dict(sigmaDepth=float("nan")), dict(sigmaLuminance=float("inf"))]
        for kw in bad:
            _expect_refusal(rtx, lambda: t.denoise_variance(**kw), "iterations|sigma|demodulate|source")
        for word in (0, 1):
            p = np.zeros((), rtx.VDENOISE_PARAMS)
            for k, v in rtx.VDENOISE_DEFAULTS.items():
                p[k] = v
            p["_reserved"][word] = 1
            assert lib.rt_denoise_variance(t._ctx, p.ctypes.data_as(ctypes.c_void_p)) == -2
            assert b"reserved" in lib.rt_last_error(t._ctx)
        n = var.size
        buf = np.empty(n + 4, np.float32)
        fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        assert lib.rt_read_variance(t._ctx, fp, n + 4) == -2 and lib.rt_read_variance(t._ctx, fp, n - 1) == -2
        assert lib.rt_read_variance(t._ctx, fp, 4 * n) == -2
        assert lib.rt_read_variance(t._ctx, None, n) == -2
        assert lib.rt_copy_variance_to_device(t._ctx, None, n) == -2
        assert lib.rt_get_vdenoise_info(t._ctx, None) == -2
        assert_same_bits(t.read_denoised(), plane, "the denoised plane after the refusals")
        assert_same_bits(t.read_variance()[..., None], var[..., None], "var_0 after the refusals")
        assert_same_full_state(full_state(t), before, "after the refusals")
        assert t.vdenoise_info() == info
        # a strip of the image: refused, naming the call that does it
        t.set_rows(8, 16)
        _expect_refusal(rtx, lambda: t.denoise_variance(), "rt_multi_denoise_variance")
    with loaded(rtx, buffers) as t:
        t.set_bands(0, 2)
        t.render(0, 1)
        t.render_aov(0, 1)
        _expect_refusal(rtx, lambda: t.denoise_variance(), "rt_multi_denoise_variance")
    for fn in ("rt_denoise_variance", "rt_get_vdenoise_info", "rt_multi_denoise_variance"):
        assert getattr(lib, fn)(None, None) == -1
    for fn in ("rt_read_variance", "rt_copy_variance_to_device", "rt_multi_read_variance"):
        assert getattr(lib, fn)(None, None, 0) == -1


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_several_contexts_give_the_single_context_result(rtx, n_ctx):
    w, h = 70, 45
    mgr, buffers = scene(rtx, "mesh_test_scene", w, h)
    params, spheres, tris, infos = buffers
    moved = temporal_check.posed(rtx, mgr, params, (0.25, 0.0, 0.0), 0.0)
    kws = {0: dict(iterations=5, demodulate=1, **TIGHT), 1: dict(DEFAULTS)}
    single = {}
    with loaded(rtx, buffers) as t:
        for k, p in enumerate((params, moved)):
            show(t, p, k)
            t.temporal()
        for source, kw in kws.items():
            t.denoise_variance(source=source, **kw)
            single[source] = (t.read_denoised(), t.read_variance(), t.read_denoised_display())
    with rtx.MultiTracer([0] * n_ctx) as m:
        m.set_params(params)
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        with pytest.raises(rtx.RtError, match="rendered|feature"):
            m.denoise_variance()
        with pytest.raises(rtx.RtError, match="rt_multi_denoise_variance has not been called"):
            m.read_variance()
        for k, p in enumerate((params, moved)):
            m.set_params(p)
            m.reset_accum()
            m.render(k, 1)
            m.reset_aov()
            m.render_aov(k, 2)
            if k == 0:
                with pytest.raises(rtx.RtError, match="rt_multi_temporal has not been called"):
                    m.denoise_variance(source=1)
            m.temporal()
        before = (m.read_accum(), m.read_aov(0), m.read_aov(1), m.read_temporal(), m.read_temporal_history()[..., None])
        for source, kw in kws.items():
            m.denoise_variance(source=source, **kw)
            assert_same_bits(m.read_denoised(), single[source][0], f"{n_ctx} contexts, source {source}: the denoised plane")
            assert_same_bits(m.read_variance()[..., None], single[source][1][..., None], f"{n_ctx} contexts, source {source}: var_0")
            np.testing.assert_array_equal(m.read_denoised_display(), single[source][2])
        after = (m.read_accum(), m.read_aov(0), m.read_aov(1), m.read_temporal(), m.read_temporal_history()[..., None])
        for a, b, what in zip(before, after, ("image", "albedo", "guide", "T", "N")):
            assert_same_bits(b, a, f"multi: {what}")
        with pytest.raises(rtx.RtError, match="iterations"):
            m.denoise_variance(iterations=9)
        assert_same_bits(m.read_denoised(), single[1][0], "after a refusal")
        n = w * h
        buf = np.empty(n + 1, np.float32)
        lib = rtx.load_library()
        assert lib.rt_multi_read_variance(m._m, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n + 1) == -2
        assert lib.rt_multi_read_variance(m._m, None, n) == -2
