"""Temporal reprojection on the GPU (rt_temporal, rt_denoise_temporal and their rt_multi forms): T and N bitwise against the lock-step
checker of tests/temporal_oracle.c, which is fed what rt_read_accum and rt_read_aov return from the same context after every call —
ragged and degenerate image sizes, two scenes, camera steps of every kind (sideways, a yaw that brings a band in from off-screen, a dolly,
none, a pose that looks away), rendered and injected colours, two tolerance sets, three history caps — and around it: the denoiser fed
from T, the context's state untouched, reset and size change, every refusal, a caller's stream, several contexts behind one handle, and
non-finite inputs."""
import ctypes

import numpy as np
import pytest

import denoise_check
import temporal_check
from aov_check import assert_same_bits
from temporal_check import DEFAULTS, TIGHT, WIDE, Checker
from test_aov_cpu import sphere_in_view
from test_gpu_aov import hip_runtime
from test_gpu_denoise import assert_same_state, inject, loaded, state_of

pytestmark = pytest.mark.gpu

# 70 x 45: ragged tiles in both axes; 200 x 120: several workgroups; 9 x 7: every bilinear footprint touches a border; one column; one row
SIZES = [(70, 45), (200, 120), (9, 7), (1, 40), (40, 1)]
# the camera steps of the four calls after call 0: (offset, yaw) from the scene's pose
STEPS = [((0.25, 0.0, 0.0), 0.0),          # sideways
         ((0.25, 0.0, 0.0), 0.35),         # a yaw far enough that a band comes from off-screen
         ((0.25, 0.0, 1.0), 0.35),         # dolly in
         ((0.25, 0.0, 1.0), 0.35),         # no motion
         ((0.25, 0.0, 1.0), np.pi)]        # looks away: every pixel without history


def scene(rtx, name, w, h, spp=2):
    """(manager, buffers)"""
    if name == "mesh_test_scene":
        mgr = rtx.scenes.mesh_test_scene(w, h)
        mgr.numRaysPerPixel = spp
        return mgr, mgr.build_buffers()
    cam = rtx.Camera(rtx.Transform(position=(0.0, 0.0, -5.0)), fieldOfView=40.0, aspect=w / h)
    mgr = rtx.RayTracingManager(cam, rtx.Light(), w, h)
    mgr.maxBounceCount, mgr.numRaysPerPixel = 2, spp
    mgr.defocusStrength, mgr.divergeStrength, mgr.focusDistance = 0.0, 1.0, 1.0
    mgr.spheres.append(rtx.RayTracedSphere(rtx.Transform(position=(0.0, 0.0, 0.0), lossyScale=(2.0, 2.0, 2.0)),
                                           rtx.RayTracingMaterial(colour=(0.25, 0.5, 0.75, 1.0))))
    return mgr, mgr.build_buffers()


def show(t, params, frame, injected_seed=None):
    """one displayed frame at a pose: fresh image and fresh feature planes"""
    t.set_params(params)
    t.reset_accum()
    t.render(frame, 1)
    t.reset_aov()
    t.render_aov(frame, 2)
    if injected_seed is not None:
        inject(t, injected_seed, hi=4.0)


def follow(rtx, t, chk, mgr, params, steps, what, injected=False, **kw):
    """call 0 at the scene's pose, then one call per step; T and N against the lock-step checker after every call"""
    poses = [params] + [temporal_check.posed(rtx, mgr, params, off, yaw) for off, yaw in steps]
    for k, p in enumerate(poses):
        show(t, p, k, injected_seed=30 + k if injected else None)
        t.temporal(**kw)
        wantT, wantN = chk.step(t.read_accum(), t.read_aov(0), t.read_aov(1), p, **dict(DEFAULTS, **kw))
        assert_same_bits(t.read_temporal(), wantT, f"{what} call {k}: T")
        assert_same_bits(t.read_temporal_history(), wantN, f"{what} call {k}: N")
    return poses


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_bitwise_against_the_checker(rtx, w, h):
    mgr, buffers = scene(rtx, "mesh_test_scene", w, h)
    with loaded(rtx, buffers) as t:
        chk = Checker()
        follow(rtx, t, chk, mgr, buffers[0], STEPS[:4], f"{w}x{h} rendered", maxHistory=32)
        info = t.temporal_info()
        assert (info["calls"], info["width"], info["height"]) == (5, w, h)
        assert info["lastKernelMs"] > 0 and info["totalKernelMs"] >= info["lastKernelMs"]
        if w * h > 1000:
            assert (chk.N > 1).mean() > 0.3                                  # (history was carried)


@pytest.mark.parametrize("tol,max_history,injected", [(WIDE, 1, False), (WIDE, 3, True), (TIGHT, 32, True), (TIGHT, 3, False)])
def test_steps_tolerances_and_caps_bitwise_against_the_checker(rtx, tol, max_history, injected):
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as t:
        chk = Checker()
        follow(rtx, t, chk, mgr, buffers[0], STEPS, f"{tol} cap {max_history}", injected=injected, maxHistory=max_history, **tol)
        assert (chk.N == 1).all() and (chk.code[..., 0] & 32 == 0).all()    # the last pose looks away


@pytest.mark.parametrize("size", [45, 64])
def test_sphere_in_view_bitwise_against_the_checker(rtx, size):
    mgr, buffers = scene(rtx, "sphere_in_view", size, size)
    with loaded(rtx, buffers) as t:
        chk = Checker()
        steps = [((0.3, 0.0, 0.0), 0.0), ((0.3, 0.0, 0.0), 0.2), ((0.3, 0.0, 1.5), 0.2), ((0.3, 0.0, 1.5), 0.2)]
        follow(rtx, t, chk, mgr, buffers[0], steps, f"sphere {size}", maxHistory=32, **WIDE)
        A = t.read_aov(0)
        assert (A[..., 3] > 0).any() and (A[..., 3] == 0).any()              # surface and sky
        assert (chk.N > 1).mean() > 0.3


def test_defaults_are_the_headers(rtx):
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as t, loaded(rtx, buffers) as spelled:
        for c, kw in ((t, {}), (spelled, DEFAULTS)):
            chk = Checker()
            follow(rtx, c, chk, mgr, buffers[0], STEPS[:2], "defaults", **kw)
        assert_same_bits(t.read_temporal(), spelled.read_temporal(), "null params against the defaults spelled out")


def test_denoise_temporal_is_the_denoiser_on_the_temporal_colour(rtx):
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as t:
        follow(rtx, t, Checker(), mgr, buffers[0], STEPS[:2], "before the denoiser")
        T = t.read_temporal()
        for kw in (dict(denoise_check.DEFAULTS), dict(iterations=3, demodulate=1, **denoise_check.TIGHT)):
            t.denoise_temporal(**kw)
            assert_same_bits(t.read_denoised(), denoise_check.checker(T, t.read_aov(0), t.read_aov(1), **kw), f"denoise_temporal {kw}")
            assert t.denoise_info()["iterations"] == kw["iterations"]
        assert_same_bits(t.read_temporal(), T, "T after the denoiser")
        # rt_denoise itself still filters resultTexture
        t.denoise(iterations=2)
        assert_same_bits(t.read_denoised(), denoise_check.checker(t.read_accum(), t.read_aov(0), t.read_aov(1),
                                                                  **dict(denoise_check.DEFAULTS, iterations=2)), "rt_denoise afterwards")


def test_the_call_moves_no_other_state_and_reset_and_resize_drop_the_history(rtx):
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    params = buffers[0]
    moved = temporal_check.posed(rtx, mgr, params, (0.2, 0.0, 0.0), 0.0)
    with loaded(rtx, buffers) as t:
        show(t, params, 0)
        t.denoise(iterations=2)
        before, dn_before = state_of(t), (t.denoise_info(), t.read_denoised())
        t.temporal()
        assert_same_state(state_of(t), before, "after rt_temporal")
        assert t.denoise_info() == dn_before[0]
        assert_same_bits(t.read_denoised(), dn_before[1], "the denoised plane")
        # the display step on T is the display step on an image with T's bits
        with loaded(rtx, buffers) as second:
            second.write_accum(t.read_temporal(), 1)
            np.testing.assert_array_equal(t.read_temporal_display(), second.read_display())
        # copy to device
        plane = t.read_temporal()
        hip, dev, back = hip_runtime(), ctypes.c_void_p(), np.zeros_like(plane)
        assert hip.hipMalloc(ctypes.byref(dev), plane.nbytes) == 0
        try:
            t.copy_temporal_to_device(dev.value, plane.size)
            assert hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), dev, plane.nbytes, 2) == 0       # device to host
        finally:
            hip.hipFree(dev)
        assert_same_bits(back, plane, "rt_copy_temporal_to_device")
        # history, then a reset: the next call is call 0 again
        show(t, moved, 1)
        t.temporal()
        assert (t.read_temporal_history() > 1).any() and t.temporal_info()["calls"] == 2
        t.reset_temporal()
        assert t.temporal_info()["calls"] == 0
        with pytest.raises(rtx.RtError, match="rt_temporal has not been called"):
            t.read_temporal()
        t.temporal()
        assert (t.read_temporal_history() == 1).all() and t.temporal_info()["calls"] == 1
        assert_same_bits(t.read_temporal(), t.read_accum(), "call 0 returns the image")
        # queued frames around the call: it settles the queue first
        t.submit_frame(2)
        t.temporal()
        assert (t.read_temporal_history() == 2).any()
    # a size change drops the history
    mgr2, buffers2 = scene(rtx, "mesh_test_scene", 48, 30)
    with loaded(rtx, buffers) as t:
        show(t, params, 0)
        t.temporal()
        show(t, params, 1)
        t.temporal()
        assert (t.read_temporal_history() == 2).any()
        show(t, buffers2[0], 2)
        t.temporal()
        assert t.read_temporal_history().shape == (30, 48) and (t.read_temporal_history() == 1).all()
        assert t.temporal_info()["calls"] == 1


def test_a_callers_stream_gives_the_same_bits(rtx):
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    with loaded(rtx, buffers) as own, loaded(rtx, buffers) as t:
        follow(rtx, own, Checker(), mgr, buffers[0], STEPS[:2], "own stream")
        hip, stream = hip_runtime(), ctypes.c_void_p()
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0 and stream.value
        try:
            t.set_stream(stream.value)
            follow(rtx, t, Checker(), mgr, buffers[0], STEPS[:2], "a caller's stream")
            got, gotN = t.read_temporal(), t.read_temporal_history()
            t.set_stream(0)
        finally:
            hip.hipStreamDestroy(stream)
        assert_same_bits(got, own.read_temporal(), "T on a caller's stream")
        assert_same_bits(gotN, own.read_temporal_history(), "N on a caller's stream")


def _expect_refusal(rtx, call, match):
    with pytest.raises(rtx.RtError, match=match) as e:
        call()
    assert "(-2)" in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was(rtx):
    lib = rtx.load_library()
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    with rtx.Tracer(0) as bare:
        _expect_refusal(rtx, lambda: bare.temporal(), "rt_set_params")
        _expect_refusal(rtx, lambda: bare.denoise_temporal(), "rt_set_params")
    with loaded(rtx, buffers) as t:
        t.render(0, 1)
        _expect_refusal(rtx, lambda: t.temporal(), "no feature frame")
        for read in (t.read_temporal, t.read_temporal_history, t.read_temporal_display):
            _expect_refusal(rtx, read, "rt_temporal has not been called")
        t.render_aov(0, 1)
        _expect_refusal(rtx, lambda: t.denoise_temporal(), "rt_temporal has not been called")
        t.temporal()
        t.temporal()
        T, N, info, before = t.read_temporal(), t.read_temporal_history(), t.temporal_info(), state_of(t)
        bad = [dict(maxHistory=0), dict(maxHistory=4097), dict(maxHistory=-1), dict(depthTolerance=0.0), dict(depthTolerance=-1.0),
               dict(normalTolerance=float("nan")), dict(normalTolerance=float("inf")), dict(depthTolerance=float("inf"))]
        for kw in bad:
            _expect_refusal(rtx, lambda: t.temporal(**kw), "maxHistory|tolerance")
        _expect_refusal(rtx, lambda: t.denoise_temporal(iterations=9), "iterations")
        n = T.size
        buf = np.empty(n + 4, np.float32)
        fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        assert lib.rt_read_temporal(t._ctx, fp, n + 4) == -2 and lib.rt_read_temporal(t._ctx, fp, n - 4) == -2
        assert lib.rt_read_temporal(t._ctx, None, n) == -2
        assert lib.rt_read_temporal_history(t._ctx, fp, n) == -2 and lib.rt_read_temporal_history(t._ctx, None, n // 4) == -2
        assert lib.rt_copy_temporal_to_device(t._ctx, None, n) == -2
        assert lib.rt_read_temporal_display(t._ctx, buf.ctypes.data_as(ctypes.c_void_p), n // 4 + 1) == -2
        assert lib.rt_read_temporal_display(t._ctx, None, n // 4) == -2
        assert lib.rt_get_temporal_info(t._ctx, None) == -2
        assert_same_bits(t.read_temporal(), T, "T after the refusals")
        assert_same_bits(t.read_temporal_history(), N, "N after the refusals")
        assert_same_state(state_of(t), before, "after the refusals")
        assert t.temporal_info() == info
        t.set_rows(8, 16)
        _expect_refusal(rtx, lambda: t.temporal(), "rt_multi_temporal")
    with loaded(rtx, buffers) as t:
        t.set_bands(0, 2)
        t.render(0, 1)
        t.render_aov(0, 1)
        _expect_refusal(rtx, lambda: t.temporal(), "rt_multi_temporal")
    for fn in ("rt_temporal", "rt_get_temporal_info", "rt_denoise_temporal", "rt_multi_temporal", "rt_multi_denoise_temporal"):
        assert getattr(lib, fn)(None, None) == -1
    for fn in ("rt_reset_temporal", "rt_multi_reset_temporal"):
        assert getattr(lib, fn)(None) == -1
    for fn in ("rt_read_temporal", "rt_read_temporal_history", "rt_copy_temporal_to_device", "rt_read_temporal_display",
               "rt_multi_read_temporal", "rt_multi_read_temporal_history", "rt_multi_read_temporal_display"):
        assert getattr(lib, fn)(None, None, 0) == -1


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_several_contexts_give_the_single_context_result(rtx, n_ctx):
    w, h = 70, 45
    mgr, buffers = scene(rtx, "mesh_test_scene", w, h)
    params, spheres, tris, infos = buffers
    poses = [params] + [temporal_check.posed(rtx, mgr, params, off, yaw) for off, yaw in STEPS[:3]]
    dkw = dict(iterations=3, demodulate=1, **denoise_check.WIDE)
    single = []
    with loaded(rtx, buffers) as t:
        for k, p in enumerate(poses):
            show(t, p, k)
            t.temporal(**WIDE)
            single.append((t.read_temporal(), t.read_temporal_history()))
        t.denoise_temporal(**dkw)
        single_denoised, single_display = t.read_denoised(), t.read_temporal_display()
    with rtx.MultiTracer([0] * n_ctx) as m:
        m.set_params(params)
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        with pytest.raises(rtx.RtError, match="rendered|feature"):
            m.temporal()
        with pytest.raises(rtx.RtError, match="rt_multi_temporal has not been called"):
            m.read_temporal()
        with pytest.raises(rtx.RtError, match="rt_multi_temporal has not been called"):
            m.denoise_temporal()
        for k, p in enumerate(poses):
            m.set_params(p)
            m.reset_accum()
            m.render(k, 1)
            m.reset_aov()
            m.render_aov(k, 2)
            image = m.read_accum()
            m.temporal(**WIDE)
            assert_same_bits(m.read_temporal(), single[k][0], f"{n_ctx} contexts call {k}: T")
            assert_same_bits(m.read_temporal_history(), single[k][1], f"{n_ctx} contexts call {k}: N")
            assert_same_bits(m.read_accum(), image, "the image after the call")
        np.testing.assert_array_equal(m.read_temporal_display(), single_display)
        m.denoise_temporal(**dkw)
        assert_same_bits(m.read_denoised(), single_denoised, f"{n_ctx} contexts: denoise_temporal")
        with pytest.raises(rtx.RtError, match="maxHistory"):
            m.temporal(maxHistory=0)
        assert_same_bits(m.read_temporal(), single[-1][0], "after a refusal")
        assert m.temporal_info()["calls"] == len(poses)
        m.reset_temporal()
        with pytest.raises(rtx.RtError, match="rt_multi_temporal has not been called"):
            m.read_temporal_history()
        m.temporal(**WIDE)
        assert (m.read_temporal_history() == 1).all()


def test_non_finite_inputs_give_the_checkers_bits(rtx):
    """arithmetic on odd data: non-finite colours in the image, then a camera matrix of NaNs, then a finite camera again (whose previous
    camera is the NaN one); every call returns 0 and matches the checker"""
    mgr, buffers = scene(rtx, "mesh_test_scene", 70, 45)
    params = buffers[0]
    with loaded(rtx, buffers) as t:
        chk = Checker()

        def call(p, what, poison=False):
            show(t, p, 0)
            if poison:
                C = t.read_accum()
                C[::5, ::7, 0], C[1::5, ::7, 1], C[2::5, ::7, 2] = np.nan, np.inf, -np.inf
                t.write_accum(C, 1)
            t.temporal(**WIDE)
            wantT, wantN = chk.step(t.read_accum(), t.read_aov(0), t.read_aov(1), p, **dict(DEFAULTS, **WIDE))
            assert_same_bits(t.read_temporal(), wantT, what + ": T")
            assert_same_bits(t.read_temporal_history(), wantN, what + ": N")
        call(params, "call 0")
        call(temporal_check.posed(rtx, mgr, params, (0.1, 0, 0), 0.0), "non-finite colours", poison=True)
        call(temporal_check.posed(rtx, mgr, params, (0.2, 0, 0), 0.0), "non-finite history")
        assert np.isnan(chk.T).any()
        nan_cam = np.array(params, dtype=rtx.PARAMS).reshape(()).copy()
        nan_cam["camLocalToWorld"] = np.nan
        t.set_params(nan_cam)
        t.temporal(**WIDE)                  # (the image and the planes of the last pose; only the camera is odd)
        wantT, wantN = chk.step(t.read_accum(), t.read_aov(0), t.read_aov(1), nan_cam, **dict(DEFAULTS, **WIDE))
        assert_same_bits(t.read_temporal(), wantT, "NaN camera: T")
        assert (wantN == 1).all() and (t.read_temporal_history() == 1).all()
        call(params, "after the NaN camera")
        assert (chk.N == 1).all()
