"""Per-frame cameras (rt_render_params, rt_submit_frame_params, rt_multi_render_params): a camera that moves between frames, traced in
shared launches, gives bit for bit what the per-frame loop rt_set_params + rt_render_frame gives — and what the oracle gives."""
import numpy as np
import pytest

from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu


def camera_path(params, n, step=0.05, turn=0.01, jump_at=None, jump=0.0):
    """n copies of params whose camera moves and turns a little every frame (position and the matrix's translation column together,
    the rotation part turned about the y axis); from frame jump_at on the camera is `jump` further along x."""
    P = np.repeat(np.asarray(params).reshape(1).copy(), n)
    M0 = np.asarray(params["camLocalToWorld"], np.float64).reshape(4, 4)
    pos0 = np.asarray(params["worldSpaceCameraPos"], np.float64)
    for f in range(n):
        a = turn * f
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        M = M0.copy()
        M[:3, :3] = R @ M0[:3, :3]
        pos = pos0 + np.array([step * f, 0.0, 0.5 * step * f])
        if jump_at is not None and f >= jump_at:
            pos[0] += jump
        M[:3, 3] = pos
        P[f]["camLocalToWorld"] = M.reshape(16).astype(np.float32)
        P[f]["worldSpaceCameraPos"] = pos.astype(np.float32)
    return P


def setup(t, b, P0, rows=None, bands=None, **options):
    params, spheres, tris, infos = b
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(P0)
    if rows is not None:
        t.set_rows(*rows)
    if bands is not None:
        t.set_bands(*bands)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    t.reset_accum()


def loop_result(rtx, b, P, first=0, **kw):
    """the per-frame loop on a context of its own"""
    with rtx.Tracer(0) as t:
        setup(t, b, P[0], **kw)
        for f in range(len(P)):
            t.set_params(P[f])
            t.render_frame(first + f)
        return t.read_accum(), t.read_last_frame(), t.stats()["numRenderedFrames"]


def batch_result(rtx, b, P, first=0, prime=True, **kw):
    with rtx.Tracer(0) as t:
        setup(t, b, P[0], **kw)
        if prime:                                   # the automatic kernel choice settles on a few static frames
            t.render(0, 4)
            t.reset_accum()
        t.render_params(first, P)
        return t.read_accum(), t.read_last_frame(), t.stats()


def assert_same(got, want, what):
    assert_bitwise(got[0], want[0], what + " resultTexture")
    assert_bitwise(got[1], want[1], what + " currentFrame")
    n = got[2]["numRenderedFrames"] if isinstance(got[2], dict) else got[2]
    assert n == want[2], (what, n, want[2])


@pytest.mark.parametrize("mode", [0, 1])
def test_orbit_equals_the_per_frame_loop_and_the_oracle(rtx, oracle, mode):
    m = rtx.scenes.mesh_test_scene(72, 40)
    b = m.build_buffers()
    params = b[0].copy(); params["intersectMode"] = mode
    b = (params,) + tuple(b[1:])
    P = camera_path(params, 16)
    want = loop_result(rtx, b, P)
    got = batch_result(rtx, b, P)
    assert_same(got, want, "orbit")
    assert got[2]["lastKernel"] == 2
    acc = None
    for f in range(16):
        cur, _ = oracle.render_frame(P[f], *b[1:], f)
        if acc is None:
            acc = np.zeros_like(cur)
        oracle.accumulate(acc, cur, f)
    assert_bitwise(got[0], acc, "orbit vs oracle resultTexture")
    assert_bitwise(got[1], cur, "orbit vs oracle currentFrame")


def test_sixteen_moving_frames_are_one_launch(rtx):
    b = rtx.scenes.mesh_test_scene(96, 64).build_buffers()
    P = camera_path(b[0], 16)
    _, _, st = batch_result(rtx, b, P)
    assert st["lastKernel"] == 2
    assert st["lastFramesPerLaunch"] == 16
    assert st["lastFramesInterleaved"] == 16
    assert st["numRenderedFrames"] == 16


def test_queued_moving_camera_is_one_launch(rtx):
    b = rtx.scenes.mesh_test_scene(72, 40).build_buffers()
    P = camera_path(b[0], 16)
    want = loop_result(rtx, b, P)
    with rtx.Tracer(0) as t:
        setup(t, b, P[0], queue_linger_us=500000)
        t.render(0, 4)
        t.reset_accum()
        for f in range(16):
            t.submit_frame_params(f, P[f])
        t.wait()
        st = t.stats()
        assert_same((t.read_accum(), t.read_last_frame(), st), want, "queued orbit")
        assert st["queuedLaunches"] == 1
        assert st["lastKernel"] == 2


def test_queued_settings_change_splits_the_queue(rtx):
    b = rtx.scenes.mesh_test_scene(72, 40).build_buffers()
    P = camera_path(b[0], 16)
    for f in range(8, 16):
        P[f]["sunIntensity"] = 3.0
        P[f]["maxBounceCount"] = 2
    want = loop_result(rtx, b, P)
    with rtx.Tracer(0) as t:
        setup(t, b, P[0], queue_linger_us=500000)
        for f in range(16):
            t.submit_frame_params(f, P[f])
        t.wait()
        st = t.stats()
        assert_same((t.read_accum(), t.read_last_frame(), st), want, "queued settings change")
        assert st["queuedLaunches"] >= 2


def test_queued_launch_error_is_reported_once(rtx):
    b = rtx.scenes.config1(32, 24).build_buffers()
    P = camera_path(b[0], 2)
    with rtx.Tracer(0) as t:
        setup(t, b, P[0], queue_linger_us=500000)
        t.render_frame(0)
        t.set_rows(20, 10)                          # rows [20, 30) of a 24-row image: checked at launch time, in the worker
        t.submit_frame_params(0, P[0]); t.submit_frame_params(1, P[1])
        with pytest.raises(rtx.RtError, match="queued frame"):
            t.wait()
        t.wait()                                    # reported once
        t.set_rows(0, 24)
        t.reset_accum()
        t.submit_frame_params(0, P[1])
        t.wait()
        assert t.stats()["numRenderedFrames"] == 1


VARIANTS = {
    "philox": dict(scene="mesh", params={"rngMode": 1}),
    "spheres_only": dict(scene="spheres", params={}, options={"kernel": 1}),      # (the automatic choice may pick k_trace without a BVH)
    "f32_nodes": dict(scene="mesh", params={}, options={"compact_nodes": 0}),
    "depth_of_field": dict(scene="mesh", params={"defocusStrength": 30.0}),
    "rows": dict(scene="mesh", params={}, rows=(16, 24)),
    "bands": dict(scene="mesh", params={}, bands=(1, 3)),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_equal_the_per_frame_loop(rtx, name):
    v = VARIANTS[name]
    m = rtx.scenes.mesh_test_scene(80, 48) if v["scene"] == "mesh" else rtx.scenes.config1(72, 40)
    b = m.build_buffers()
    params = b[0].copy()
    for k, x in v["params"].items():
        params[k] = x
    b = (params,) + tuple(b[1:])
    P = camera_path(params, 16)
    kw = dict(v.get("options", {}))
    if "rows" in v:
        kw["rows"] = v["rows"]
    if "bands" in v:
        kw["bands"] = v["bands"]
    want = loop_result(rtx, b, P, first=3, **kw)
    got = batch_result(rtx, b, P, first=3, **kw)
    assert_same(got, want, name)
    assert got[2]["lastKernel"] == 2, name


def test_padding_widens_mid_batch(rtx):
    b = rtx.scenes.mesh_test_scene(72, 40).build_buffers()
    P = camera_path(b[0], 16, jump_at=8, jump=2000.0)
    want = loop_result(rtx, b, P)
    got = batch_result(rtx, b, P)
    assert_same(got, want, "camera far out from frame 8")
    assert got[2]["bvhRepads"] >= 1


def test_identical_cameras_take_the_static_path(rtx):
    b = rtx.scenes.mesh_test_scene(96, 64).build_buffers()
    P = np.repeat(np.asarray(b[0]).reshape(1).copy(), 16)
    with rtx.Tracer(0) as t:
        setup(t, b, P[0])
        t.render(0, 4)
        t.reset_accum()
        t.render(0, 16)
        want = (t.read_accum(), t.read_last_frame(), t.stats()["numRenderedFrames"])
        t.reset_accum()
        moved = P.copy()                            # lists for another camera in between
        for q in moved:
            q["worldSpaceCameraPos"] = q["worldSpaceCameraPos"] + np.float32(0.25)
        t.render_params(0, moved)
        t.reset_accum()
        builds = t.stats()["primaryListBuilds"]
        t.render_params(0, P)
        st = t.stats()
        assert_same((t.read_accum(), t.read_last_frame(), st), want, "identical cameras")
        assert st["lastKernel"] == 1
        assert st["primaryListBuilds"] > builds


def test_mismatched_settings_are_refused_and_change_nothing(rtx):
    b = rtx.scenes.mesh_test_scene(72, 40).build_buffers()
    P = camera_path(b[0], 4)
    with rtx.Tracer(0) as t:
        setup(t, b, P[0])
        t.render_params(0, P[:2])
        acc, last, n = t.read_accum(), t.read_last_frame(), t.stats()["numRenderedFrames"]
        bad = camera_path(b[0], 4, step=0.3)
        bad[2]["numRaysPerPixel"] = 1
        rc = t._lib.rt_render_params(t._ctx, 2, 4, np.ascontiguousarray(bad).ctypes.data)
        assert rc == -2
        assert_same((t.read_accum(), t.read_last_frame(), t.stats()["numRenderedFrames"]), (acc, last, n), "after the refused call")
        t.render_frame(2)                           # the context's params are still P[1]
        got = (t.read_accum(), t.read_last_frame(), t.stats()["numRenderedFrames"])
    with rtx.Tracer(0) as u:
        setup(u, b, P[0])
        u.render_params(0, P[:2])
        u.render_frame(2)
        want = (u.read_accum(), u.read_last_frame(), u.stats()["numRenderedFrames"])
    assert_same(got, want, "params unchanged by the refused call")


def test_multi_render_params_equals_one_context(rtx):
    b = rtx.scenes.mesh_test_scene(80, 48).build_buffers()
    params, spheres, tris, infos = b
    P = camera_path(params, 16)
    want = batch_result(rtx, b, P)
    with rtx.MultiTracer([0, 0]) as m:
        m.set_params(P[0])
        m.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        m.reset_accum()
        m.render_params(0, P)
        assert_bitwise(m.read_accum(), want[0], "rt_multi_render_params resultTexture")
