"""The denoiser on the GPU (rt_denoise and rt_multi_denoise): the denoised plane bitwise against tests/denoise_oracle.c, which is fed what
rt_read_accum and rt_read_aov return from the same context — rendered and injected colours, ragged and degenerate image sizes, every
iteration count that takes another path, both demodulation settings, a wide and a tight sigma set — and around it: the context's state
untouched, the display step, every refusal, several contexts behind one handle, and the error of a noisy render reduced."""
import ctypes

import numpy as np
import pytest

import denoise_check
from aov_check import assert_same_bits
from denoise_check import DEFAULTS, TIGHT, WIDE
from test_aov_cpu import sphere_in_view
from test_gpu_aov import hip_runtime

pytestmark = pytest.mark.gpu

# 70 x 45: ragged tiles in both axes, a height that is no multiple of 8; 200 x 120: several workgroups; 9 x 7: with 6 iterations every
# off-centre tap of the late passes lies outside; one column; one row
SIZES = [(70, 45), (200, 120), (9, 7), (1, 40), (40, 1)]


def buffers_of(rtx, scene, w, h, spp=2):
    if scene == "mesh_test_scene":
        mgr = rtx.scenes.mesh_test_scene(w, h)
        mgr.numRaysPerPixel = spp
        return mgr.build_buffers()
    assert w == h
    b = sphere_in_view(rtx, n=spp, diverge=1.0, size=w)
    return b


def loaded(rtx, buffers):
    params, spheres, tris, infos = buffers
    t = rtx.Tracer(0)
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    return t


def prepared(rtx, scene, w, h, frames=1, aov_frames=2):
    """a context with `frames` image frames and `aov_frames` feature frames"""
    t = loaded(rtx, buffers_of(rtx, scene, w, h))
    if frames:
        t.render(0, frames)
    t.render_aov(0, aov_frames)
    return t


def inject(t, seed, hi=1e4):
    H, W = int(t._params["height"]), int(t._params["width"])
    C = np.random.default_rng(seed).uniform(0.0, hi, (H, W, 4)).astype(np.float32)
    t.write_accum(C, 3)
    return C


def want_of(t, **kw):
    return denoise_check.checker(t.read_accum(), t.read_aov(0), t.read_aov(1), **kw)


def state_of(t):
    return {"accum": t.read_accum(), "last": t.read_last_frame(), "albedo": t.read_aov(0), "guide": t.read_aov(1),
            "stats": t.stats(), "aov_info": t.aov_info()}


def assert_same_state(a, b, what):
    for k in ("accum", "last", "albedo", "guide"):
        assert_same_bits(a[k], b[k], f"{what}: {k}")
    assert a["stats"] == b["stats"], (what, {k: (a["stats"][k], b["stats"][k]) for k in a["stats"] if a["stats"][k] != b["stats"][k]})
    assert a["aov_info"] == b["aov_info"], what


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_bitwise_against_the_checker(rtx, w, h):
    """mesh_test_scene's guides (silhouettes, sky, a checker floor, invisible lights); the rendered image, then injected colours"""
    with prepared(rtx, "mesh_test_scene", w, h) as t:
        for colour in ("rendered", "injected"):
            if colour == "injected":
                inject(t, 7)
            for iterations, demod, sig in ((1, 1, WIDE), (2, 0, TIGHT), (5, 1, TIGHT), (6, 1, WIDE), (6, 0, WIDE)):
                kw = dict(iterations=iterations, demodulate=demod, **sig)
                t.denoise(**kw)
                assert_same_bits(t.read_denoised(), want_of(t, **kw), f"{w}x{h} {colour} {kw}")
                info = t.denoise_info()
                assert (info["iterations"], info["demodulate"], info["width"], info["height"]) == (iterations, demod, w, h)
                assert info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"]


@pytest.mark.parametrize("size", [45, 64])
def test_sphere_in_view_bitwise_against_the_checker(rtx, size):
    with prepared(rtx, "sphere_in_view", size, size) as t:
        A = t.read_aov(0)
        assert ((A[..., 3] > 0) & (A[..., 3] < 1)).any() and (A[..., 3] == 0).any()          # a silhouette and sky
        for colour in ("rendered", "injected"):
            if colour == "injected":
                inject(t, 8)
            for iterations, demod, sig in ((1, 0, TIGHT), (2, 1, WIDE), (5, 0, WIDE), (6, 1, TIGHT)):
                kw = dict(iterations=iterations, demodulate=demod, **sig)
                t.denoise(**kw)
                assert_same_bits(t.read_denoised(), want_of(t, **kw), f"sphere {size} {colour} {kw}")


def test_defaults_are_the_headers(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        t.denoise()
        got = t.read_denoised()
        assert_same_bits(got, want_of(t, **DEFAULTS), "null params")
        t.denoise(**DEFAULTS)
        assert_same_bits(t.read_denoised(), got, "the defaults spelled out")
        assert t.denoise_info()["iterations"] == DEFAULTS["iterations"]


def test_the_call_moves_no_other_state(rtx):
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as t, loaded(rtx, buffers) as plain:
        for c in (t, plain):
            c.render(0, 2)
            c.render_aov(0, 1)
        before = state_of(t)
        t.denoise(iterations=3)
        first = t.read_denoised()
        assert_same_state(state_of(t), before, "after rt_denoise")
        t.denoise(iterations=3)
        assert_same_bits(t.read_denoised(), first, "a second call")
        # a frame rendered afterwards equals the same frame without the call
        t.render(2, 1)
        plain.render(2, 1)
        assert_same_bits(t.read_accum(), plain.read_accum(), "frame 2 after the call")
        assert_same_bits(t.read_last_frame(), plain.read_last_frame(), "currentFrame of frame 2")
        assert t.stats()["numRenderedFrames"] == plain.stats()["numRenderedFrames"] == 3
        # interleaved with queued frames: the call settles the queue first, and the queue goes on after it
        for c in (t, plain):
            c.submit_frame(3)
            c.submit_frame(4)
        t.denoise(iterations=2)
        assert_same_bits(t.read_denoised(), want_of(t, iterations=2, **{k: DEFAULTS[k] for k in ("demodulate", "sigmaColour", "sigmaNormal", "sigmaDepth")}),
                         "after two queued frames")
        for c in (t, plain):
            c.submit_frame(5)
            c.wait()
        assert_same_bits(t.read_accum(), plain.read_accum(), "queued frames around the call")
        assert t.stats()["numRenderedFrames"] == plain.stats()["numRenderedFrames"] == 6


def test_a_callers_stream_gives_the_same_bits(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        t.denoise(iterations=4)
        own = t.read_denoised()
        hip, stream = hip_runtime(), ctypes.c_void_p()
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        try:
            t.set_stream(stream.value)
            t.denoise(iterations=4)
            got = t.read_denoised()
            t.set_stream(0)
        finally:
            hip.hipStreamDestroy(stream)
        assert_same_bits(got, own, "on a caller's stream")


def test_copy_to_device_is_the_plane(rtx):
    with prepared(rtx, "mesh_test_scene", 70, 45) as t:
        t.denoise(iterations=2)
        plane = t.read_denoised()
        hip, dev, back = hip_runtime(), ctypes.c_void_p(), np.zeros_like(plane)
        assert hip.hipMalloc(ctypes.byref(dev), plane.nbytes) == 0
        try:
            t.copy_denoised_to_device(dev.value, plane.size)
            assert hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), dev, plane.nbytes, 2) == 0       # device to host
        finally:
            hip.hipFree(dev)
        assert_same_bits(back, plane, "rt_copy_denoised_to_device")


def test_display_is_the_existing_display_step_on_the_denoised_plane(rtx):
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with prepared(rtx, "mesh_test_scene", 70, 45, frames=2) as t, loaded(rtx, buffers) as second:
        t.denoise()
        second.write_accum(t.read_denoised(), 1)
        np.testing.assert_array_equal(t.read_denoised_display(), second.read_display())
        assert t.read_denoised_display()[..., :3].any()


def _expect_refusal(rtx, t, call, match, lib_call=None):
    with pytest.raises(rtx.RtError, match=match) as e:
        call()
    assert "(-2)" in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was(rtx):
    lib = rtx.load_library()
    buffers = buffers_of(rtx, "mesh_test_scene", 70, 45)
    with rtx.Tracer(0) as bare:
        _expect_refusal(rtx, bare, lambda: bare.denoise(), "rt_set_params")
    with loaded(rtx, buffers) as t:
        t.render(0, 1)
        _expect_refusal(rtx, t, lambda: t.denoise(), "no feature frame")
        _expect_refusal(rtx, t, lambda: t.read_denoised(), "rt_denoise has not been called")
        _expect_refusal(rtx, t, lambda: t.read_denoised_display(), "rt_denoise has not been called")
        t.render_aov(0, 1)
        t.denoise(iterations=2)
        plane, before = t.read_denoised(), state_of(t)
        info = t.denoise_info()
        bad = [dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(demodulate=2),
               dict(sigmaColour=0.0), dict(sigmaNormal=-1.0), dict(sigmaDepth=float("nan")), dict(sigmaColour=float("inf"))]
        for kw in bad:
            _expect_refusal(rtx, t, lambda: t.denoise(**kw), "iterations|sigma|demodulate")
        n = plane.size
        buf = np.empty(n + 4, np.float32)
        fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        assert lib.rt_read_denoised(t._ctx, fp, n + 4) == -2 and lib.rt_read_denoised(t._ctx, fp, n - 4) == -2
        assert lib.rt_read_denoised(t._ctx, None, n) == -2
        assert lib.rt_copy_denoised_to_device(t._ctx, None, n) == -2
        assert lib.rt_read_denoised_display(t._ctx, buf.ctypes.data_as(ctypes.c_void_p), n // 4 + 1) == -2
        assert lib.rt_read_denoised_display(t._ctx, None, n // 4) == -2
        assert lib.rt_get_denoise_info(t._ctx, None) == -2
        assert_same_bits(t.read_denoised(), plane, "the denoised plane after the refusals")
        assert_same_state(state_of(t), before, "after the refusals")
        assert t.denoise_info() == info
        # a strip of the image: refused, naming the call that does it
        t.set_rows(8, 16)
        _expect_refusal(rtx, t, lambda: t.denoise(), "rt_multi_denoise")
    with loaded(rtx, buffers) as t:
        t.set_bands(0, 2)
        t.render(0, 1)
        t.render_aov(0, 1)
        _expect_refusal(rtx, t, lambda: t.denoise(), "rt_multi_denoise")
    for fn in ("rt_denoise", "rt_get_denoise_info", "rt_multi_denoise"):
        assert getattr(lib, fn)(None, None) == -1
    for fn in ("rt_read_denoised", "rt_copy_denoised_to_device", "rt_read_denoised_display", "rt_multi_read_denoised", "rt_multi_read_denoised_display"):
        assert getattr(lib, fn)(None, None, 0) == -1


@pytest.mark.parametrize("n_ctx", [2, 3])
@pytest.mark.parametrize("w,h", [(70, 45), (200, 120)])
def test_several_contexts_give_the_single_context_plane(rtx, n_ctx, w, h):
    buffers = buffers_of(rtx, "mesh_test_scene", w, h)
    params, spheres, tris, infos = buffers
    kw = dict(iterations=5, demodulate=1, **TIGHT)
    with loaded(rtx, buffers) as t:
        t.render(0, 2)
        t.render_aov(0, 2)
        t.denoise(**kw)
        single, single_display = t.read_denoised(), t.read_denoised_display()
    lib = rtx.load_library()
    with rtx.MultiTracer([0] * n_ctx) as m:
        m.set_params(params)
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        with pytest.raises(rtx.RtError, match="rendered|feature"):
            m.denoise(**kw)
        m.render(0, 2)
        with pytest.raises(rtx.RtError, match="no feature frame"):
            m.denoise(**kw)
        with pytest.raises(rtx.RtError, match="rt_multi_denoise has not been called"):
            m.read_denoised()
        m.render_aov(0, 2)

        def per_context():
            out = []
            for i in range(n_ctx):
                c = lib.rt_multi_context(m._m, i)
                s, a = np.zeros((), rtx.STATS), np.zeros((), rtx.AOV_INFO)
                assert lib.rt_get_stats(c, s.ctypes.data_as(ctypes.c_void_p)) == 0 and lib.rt_get_aov_info(c, a.ctypes.data_as(ctypes.c_void_p)) == 0
                out.append((s.tobytes(), a.tobytes()))
            return out
        before = (m.read_accum(), m.read_aov(0), m.read_aov(1), per_context())
        m.denoise(**kw)
        assert_same_bits(m.read_denoised(), single, f"{n_ctx} contexts {w}x{h}")
        np.testing.assert_array_equal(m.read_denoised_display(), single_display)
        after = (m.read_accum(), m.read_aov(0), m.read_aov(1), per_context())
        for a, b, what in zip(before[:3], after[:3], ("image", "albedo", "guide")):
            assert_same_bits(b, a, f"multi: {what}")
        assert before[3] == after[3]
        with pytest.raises(rtx.RtError, match="iterations"):
            m.denoise(iterations=9)
        assert_same_bits(m.read_denoised(), single, "after a refusal")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("spp", [1, 4])
def test_denoised_render_is_closer_to_a_many_frame_render(rtx, spp, mode):
    """96 x 64, the defaults: RMSE(denoised) < RMSE(noisy), both against 16 frames of 64 samples per pixel of the same tracer"""
    def buffers(n):
        mgr = rtx.scenes.mesh_test_scene(96, 64)
        mgr.numRaysPerPixel = n
        b = mgr.build_buffers()
        b[0]["rngMode"] = mode
        return b
    with loaded(rtx, buffers(64)) as ref:
        ref.render(1000, 16)
        converged = ref.read_accum()
    with loaded(rtx, buffers(spp)) as t:
        t.render(0, 1)
        t.render_aov(0, 4)
        t.denoise()
        noisy, den = t.read_accum(), t.read_denoised()
    before, after = denoise_check.rmse(noisy, converged), denoise_check.rmse(den, converged)
    print(f"{spp} spp, rngMode {mode}: RMSE noisy {before:.4f}, denoised {after:.4f}, ratio {after / before:.3f}")
    assert after < before
