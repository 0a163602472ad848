"""Temporal reprojection without a GPU: the checker (tests/temporal_oracle.c) is pinned to a float64 restatement of the definition and to
analytic cases, the definition is shown to beat both a single noisy frame and plain accumulation along a camera path, and the ABI is
declared, exported and bound.

(a) Float64 twin.  temporal_check.Twin64 restates include/rt.h's text in float64.  Both start from the same previous state (random T',
    N' in 0..40, the guide of other random planes) and take one step over a random rigid camera pair.  A pixel whose decisions (valid,
    the tap origin, which taps count, sw >= 0.01, the cap) agree must match within the tolerance DESIGN.md "Temporal reprojection"
    derives: the reprojection chain has at most 33 roundings, so px and py are off by at most E = 33 * 2^-24 * px_scale pixels
    (px_scale: the magnitudes that enter the chain over the depth in the previous camera, in pixels); the history is a weighted mean
    of the taps, whose derivative in (px, py) is at most 8 * range / sw; the blend itself adds at most 16 roundings of range.
    Decisions may differ only where a quantity lies within its rounding band of a threshold: a pixel takes about 20 such decisions,
    each band is below 1e-4 of the quantity's range here, so at most 0.2 % of the pixels are expected to differ; the cap asserted
    is 0.5 %.  Three deliberate misreadings (clamped taps, no depth test, no cap) must fail the same comparison.
(b) Analytic cases: a static camera gives the running mean, maxHistory 1 gives C, a sideways step of one pixel's footprint in front of
    a fronto-parallel plane shifts the history by one pixel, a sphere in front of a plane leaves disoccluded background without
    history, a rotation in front of sky carries the history along the direction, a point behind the previous camera has none.
(c) mesh_test_scene at 96 x 64 along a path of 8 poses: RMSE of T against a converged render of the last pose below the single
    frame's and below plain accumulation's, and T + denoiser below frame + denoiser.
(d) The boundary: symbols, struct sizes and field orders, the three host layers, the kernel's resources."""
import os
import re

import numpy as np
import pytest

import aov_check
import denoise_check
import temporal_check
from temporal_check import Checker, Twin64, rigid_camera
from test_camera_batch_cpu import built_library
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_temporal", "rt_reset_temporal", "rt_read_temporal", "rt_read_temporal_history", "rt_copy_temporal_to_device",
           "rt_read_temporal_display", "rt_get_temporal_info", "rt_denoise_temporal",
           "rt_multi_temporal", "rt_multi_reset_temporal", "rt_multi_read_temporal", "rt_multi_read_temporal_history",
           "rt_multi_read_temporal_display", "rt_multi_denoise_temporal")

EPS = 2.0 ** -23
TWIN_W, TWIN_H = 37, 23
TWIN_ROUNDINGS = 33                 # of the chain from (x, y) to (px, py), each at most half an ulp
TWIN_DECISION_CAP = 0.005           # share of pixels whose decisions may differ
TWIN_CASES = [(seed, tol, mh) for seed in (11, 12, 13) for tol, mh in (("WIDE", 32), ("WIDE", 4), ("DEFAULTS", 32))]


def _twin_pair(seed, tol, max_history, variant=0):
    """(checker, twin) after one step from the same injected state"""
    C0, A0, G0 = denoise_check.random_inputs(TWIN_W, TWIN_H, seed)
    C1, A1, G1 = denoise_check.random_inputs(TWIN_W, TWIN_H, seed + 100)
    rng = np.random.default_rng(seed)
    cam0, cam1 = temporal_check.random_camera_pair(seed)
    kw = dict(getattr(temporal_check, tol), maxHistory=max_history)
    kw = {k: kw[k] for k in ("maxHistory", "depthTolerance", "normalTolerance")}
    # the previous state: what a call over (C0, A0, G0) leaves, with the history lengths replaced by random ones (0 = never written)
    chk, twin = Checker(), Twin64()
    chk.step(C0, A0, G0, cam0, **kw)
    twin.step(C0, A0, G0, cam0, **kw)
    N = rng.integers(0, 41, (TWIN_H, TWIN_W)).astype(np.float32)
    chk.N, twin.N = N.copy(), N.astype(np.float64)
    chk.step(C1, A1, G1, cam1, variant=variant, **kw)
    twin.step(C1, A1, G1, cam1, **kw)
    return chk, twin, C1


def _twin_compare(chk, twin, C1):
    """(share of pixels whose decisions differ, share of pixels with history, largest error / tolerance over the agreeing pixels)"""
    agree = (chk.code == twin.code).all(-1)
    hist = (twin.code[..., 0] & 32) != 0
    E = TWIN_ROUNDINGS * EPS / 2 * twin.px_scale
    sw = np.where(hist, twin.sw, 1.0)
    tol_T = np.where(hist, 8.0 * E * 1.0 / sw + 16 * EPS * 1.0, 0.0)            # colours in [0, 1]
    tol_N = np.where(hist, 8.0 * E * 40.0 / sw + 16 * EPS * 41.0, 0.0)          # history lengths in [0, 40]
    err_T = np.abs(chk.T.astype(np.float64) - twin.T)[..., :3].max(-1)
    err_N = np.abs(chk.N.astype(np.float64) - twin.N)
    m = agree & hist
    worst = max(float((err_T[m] / tol_T[m]).max()), float((err_N[m] / tol_N[m]).max())) if m.any() else 0.0
    # without history the result is the input's bits
    nohist = agree & ~hist
    assert (chk.T[nohist] == C1[nohist]).all() and (chk.N[nohist] == 1).all()
    return 1.0 - agree.mean(), hist.mean(), worst


@pytest.mark.parametrize("seed,tol,max_history", TWIN_CASES)
def test_checker_agrees_with_the_float64_twin(seed, tol, max_history):
    chk, twin, C1 = _twin_pair(seed, tol, max_history)
    differ, with_history, worst = _twin_compare(chk, twin, C1)
    print(f"seed {seed}, {tol}, maxHistory {max_history}: decisions differ on {differ:.4%}, history on {with_history:.1%}, "
          f"largest error / tolerance {worst:.3f}")
    assert differ <= TWIN_DECISION_CAP
    assert worst <= 1.0
    if tol == "WIDE":
        assert with_history > 0.2                   # (the comparison is about pixels that blend)
    np.testing.assert_array_equal(chk.T[..., 3], C1[..., 3])


@pytest.mark.parametrize("variant,max_history", [(1, 32), (2, 32), (3, 4)])
def test_misreadings_of_the_definition_fail_the_twin_comparison(variant, max_history):
    """taps clamped instead of skipped (1), no depth test (2), a history length that is not capped (3)"""
    failed = 0
    for seed in (11, 12, 13):
        chk, twin, C1 = _twin_pair(seed, "WIDE", max_history, variant=variant)
        differ, _, worst = _twin_compare(chk, twin, C1)
        failed += differ > TWIN_DECISION_CAP or worst > 1.0
    assert failed == 3


# ---- (b) analytic cases ----------------------------------------------------------------------------------------------------------------
VIEW = (1.2, 0.8, 1.0)


def _rays(W, H, cam):
    """float64 centre rays of a camera: (origin, directions [H, W, 3])"""
    M, O, V = (a.astype(np.float64) for a in temporal_check.camera_of(cam))
    ys, xs = np.mgrid[0:H, 0:W]
    l = np.stack([((xs + 0.5) / W - 0.5) * V[0], ((ys + 0.5) / H - 0.5) * V[1], np.full((H, W), V[2]), np.ones((H, W))], -1)
    d = l @ M.reshape(4, 4)[:3].T - O
    return O, d / np.linalg.norm(d, axis=-1, keepdims=True)


def _plane_guides(W, H, cam, z_plane, sphere=None):
    """(A, G) of a plane z = z_plane facing -z, optionally with a sphere (centre, radius) in front of it"""
    O, d = _rays(W, H, cam)
    depth = (z_plane - O[2]) / d[..., 2]
    normal = np.broadcast_to(np.array([0.0, 0.0, -1.0]), d.shape).copy()
    if sphere is not None:
        c, r = np.asarray(sphere[0], np.float64), sphere[1]
        oc = O - c
        b = (d * oc).sum(-1)
        disc = b * b - ((oc * oc).sum() - r * r)
        hit = disc > 0
        t = -b - np.sqrt(np.where(hit, disc, 0.0))
        hit &= t > 0
        depth = np.where(hit, t, depth)
        normal = np.where(hit[..., None], (O + d * t[..., None] - c) / r, normal)
    A = np.ones((H, W, 4), np.float32)
    G = np.concatenate([normal, depth[..., None]], -1).astype(np.float32)
    return A, G


def test_a_static_camera_gives_the_running_mean():
    """Camera at the origin with the identity rotation: F = l exactly, and the chain to px has 7 roundings of quantities of at most 1/2
    before the scale by W: |px - x| <= 3 * W * eps.  A call leaks at most 2 * 3 * W * eps * range from the neighbours and rounds 4
    times; k calls at most k times that.  The history length of equal taps is k up to the rounding of b * N' (4 eps)."""
    W, H, k = 32, 20, 6
    cam = rigid_camera((0, 0, 0), view=VIEW)
    A, G = _plane_guides(W, H, cam, 5.0)
    rng = np.random.default_rng(3)
    chk, mean = Checker(), np.zeros((H, W, 3))
    for call in range(k):
        C = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
        T, N = chk.step(C, A, G, cam, maxHistory=4096)
        mean += (C[..., :3].astype(np.float64) - mean) / (call + 1)
        tol = (call + 1) * (6 * W * EPS + 4 * EPS)
        err = np.abs(T[..., :3] - mean).max()
        print(f"call {call}: max |T - mean| {err:.3e}, tolerance {tol:.3e}; N in [{N.min()}, {N.max()}]")
        assert err <= tol
        assert np.abs(N - (call + 1)).max() <= 4 * EPS * (call + 1)
        np.testing.assert_array_equal(T[..., 3], C[..., 3])


def test_max_history_one_returns_the_input():
    W, H = 32, 20
    cam0, cam1 = temporal_check.random_camera_pair(5)
    chk = Checker()
    for call, cam in enumerate((cam0, cam1, cam1)):
        C, A, G = denoise_check.random_inputs(W, H, 20 + call)
        T, N = chk.step(C, A, G, cam, **dict(temporal_check.WIDE, maxHistory=1))
        aov_check.assert_same_bits(T, C, f"call {call}")
        assert (N == 1).all()
    assert (chk.code[..., 0] & 32).any()            # (there was history to blend: the cap made it weigh nothing)


def test_a_sideways_step_of_one_pixel_shifts_the_history_by_one_pixel():
    """A plane z = d seen from the origin; the camera moves along +x by the footprint of a pixel at that depth, (V.x / W) * d / V.z:
    pixel x now sees what pixel x + 1 saw.  With maxHistory large, T1(x) = T0(x + 1) / 2 + C1(x) / 2; the last column sees a part of
    the plane that was outside and has no history.  Tolerance: |px - (x + 1)| <= 16 * W * eps (the chain now carries the camera's
    offset, of the size of a pixel), leaking 2 * that * range, plus 4 roundings."""
    W, H, d = 32, 20, 5.0
    step = VIEW[0] / W * d / VIEW[2]
    cam0, cam1 = rigid_camera((0, 0, 0), view=VIEW), rigid_camera((step, 0, 0), view=VIEW)
    rng = np.random.default_rng(4)
    C0, C1 = (rng.uniform(0, 1, (H, W, 4)).astype(np.float32) for _ in range(2))
    chk = Checker()
    T0, _ = chk.step(C0, *_plane_guides(W, H, cam0, d), cam0, maxHistory=4096)
    T1, N1 = chk.step(C1, *_plane_guides(W, H, cam1, d), cam1, maxHistory=4096)
    want = 0.5 * T0[:, 1:, :3].astype(np.float64) + 0.5 * C1[:, :-1, :3]
    err, tol = np.abs(T1[:, :-1, :3] - want).max(), 32 * W * EPS + 4 * EPS
    print(f"max |T1 - shifted| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert (N1[:, :-1] == 2).all() and (N1[:, -1] == 1).all()
    aov_check.assert_same_bits(np.ascontiguousarray(T1[:, -1]), np.ascontiguousarray(C1[:, -1]), "the entering column")


def test_background_that_was_hidden_has_no_history():
    """A sphere (radius 1 at z = 4) in front of a plane z = 8, the camera moved sideways by 0.6: the plane points the sphere hid from
    the first camera (by a margin of two pixels) come out with N == 1 under the defaults; plane points seen by both, away from the
    silhouette and inside the first view, keep their history."""
    W, H = 64, 40
    centre, radius = (0.0, 0.0, 4.0), 1.0
    cam0, cam1 = rigid_camera((0, 0, 0), view=VIEW), rigid_camera((0.6, 0, 0), view=VIEW)
    (A0, G0), (A1, G1) = (_plane_guides(W, H, c, 8.0, (centre, radius)) for c in (cam0, cam1))
    rng = np.random.default_rng(6)
    chk = Checker()
    chk.step(rng.uniform(0, 1, (H, W, 4)).astype(np.float32), A0, G0, cam0)
    _, N = chk.step(rng.uniform(0, 1, (H, W, 4)).astype(np.float32), A1, G1, cam1)
    O1, d1 = _rays(W, H, cam1)
    on_plane = G1[..., 2] == -1
    X = O1 + d1 * G1[..., 3:4].astype(np.float64)                               # the points seen now
    # from the first camera (at the origin, looking along z): the angle to the sphere's centre against its angular radius
    to_c = np.asarray(centre) / np.linalg.norm(centre)
    cos_a = (X @ to_c) / np.linalg.norm(X, axis=-1)
    ang, ang_sphere = np.arccos(np.clip(cos_a, -1, 1)), np.arcsin(radius / np.linalg.norm(centre))
    pixel = VIEW[0] / W                                                          # (about the angle of a pixel)
    hidden = on_plane & (ang < ang_sphere - 2 * pixel)
    px0 = (X[..., 0] / X[..., 2] / VIEW[0] + 0.5) * W - 0.5
    seen = on_plane & (ang > ang_sphere + 2 * pixel) & (px0 > 1) & (px0 < W - 2)
    print(f"{hidden.sum()} disoccluded pixels, {seen.sum()} plane pixels seen by both")
    assert hidden.sum() > 20 and seen.sum() > 500
    assert (N[hidden] == 1).all()
    assert (N[seen] == 2).all()


def test_a_rotation_in_front_of_sky_carries_the_history_along_the_direction():
    """Pure sky (coverage 0), the first image a linear function of the view direction, the second input black: 2 * T1 is the history,
    the bilinear interpolation of the first image where the direction was.  f = 0.5 + 0.5 * dir has second derivatives below
    (V.x / W)^2 per pixel^2, so the interpolation error where all four taps lie inside is below 2 * (1 / 8) * (V.x / W)^2 = 1e-4 at W = 64,
    V.x = 1.2; directions that were outside the first view (a band on the side the camera turned to) have no history."""
    W, H, yaw = 64, 40, 0.2
    cam0, cam1 = rigid_camera((0.3, -0.2, 0.5), view=VIEW), rigid_camera((1.3, 0.8, -2.5), yaw=yaw, view=VIEW)     # (translation is ignored)
    A = np.zeros((H, W, 4), np.float32)
    G = np.zeros((H, W, 4), np.float32)
    _, d0 = _rays(W, H, cam0)
    _, d1 = _rays(W, H, cam1)
    C0 = np.concatenate([0.5 + 0.5 * d0, np.ones((H, W, 1))], -1).astype(np.float32)
    chk = Checker()
    chk.step(C0, A, G, cam0, maxHistory=4096)
    T1, N1 = chk.step(np.zeros((H, W, 4), np.float32), A, G, cam1, maxHistory=4096)
    had = N1 == 2
    R0 = temporal_check.camera_of(cam0)[0].astype(np.float64).reshape(4, 4)[:3, :3]
    local = d1 @ R0                                                              # the new directions in the first camera
    px0 = (local[..., 0] / local[..., 2] / VIEW[0] + 0.5) * W - 0.5
    py0 = (local[..., 1] / local[..., 2] / VIEW[1] + 0.5) * H - 0.5
    interior = (px0 >= 0) & (px0 <= W - 1) & (py0 >= 0) & (py0 <= H - 1)        # all four taps inside the first image
    outside = (px0 <= -1) | (px0 >= W) | (py0 <= -1) | (py0 >= H)
    assert had[interior].all() and not had[outside].any()
    assert interior.sum() > W * H // 2 and outside.sum() >= H * 5
    err = np.abs(2.0 * T1[interior][:, :3] - (0.5 + 0.5 * d1[interior])).max()
    tol = 0.25 * (VIEW[0] / W) ** 2 + 64 * EPS
    print(f"{interior.mean():.1%} of the pixels have all four taps; max |2 T1 - f(dir)| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert (N1[~had] == 1).all() and (T1[~had][:, :3] == 0).all()


@pytest.mark.parametrize("kind", ["sky", "surface"])
def test_a_point_behind_the_previous_camera_has_no_history(kind):
    W, H = 32, 20
    rng = np.random.default_rng(8)
    C0, C1 = (rng.uniform(0, 1, (H, W, 4)).astype(np.float32) for _ in range(2))
    if kind == "sky":
        cam0, cam1 = rigid_camera((0, 0, 0), view=VIEW), rigid_camera((0, 0, 0), yaw=np.pi, view=VIEW)
        g0 = g1 = (np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32))
    else:                                           # a plane one unit in front of the second camera, the first camera beyond it
        cam0, cam1 = rigid_camera((0, 0, 3), view=VIEW), rigid_camera((0, 0, 0), view=VIEW)
        g0, g1 = _plane_guides(W, H, cam0, 9.0), _plane_guides(W, H, cam1, 1.0)
    chk = Checker()
    chk.step(C0, *g0, cam0, **temporal_check.WIDE)
    T1, N1 = chk.step(C1, *g1, cam1, **temporal_check.WIDE)
    assert (chk.code[..., 0] == 0).all()
    aov_check.assert_same_bits(T1, C1, kind)
    assert (N1 == 1).all()


# ---- (c) quality of the definition -----------------------------------------------------------------------------------------------------
QW, QH, POSES = 96, 64, 8
PATH_STEP, PATH_YAW = (0.12, 0.0, 0.05), -0.01      # per pose: sideways and a little forward, turning slightly against the motion


# The denoiser after the step: five passes with a colour sigma of the size of the noise (0.5 on colours in [0, 1]; the sigmas the
# denoiser's own twin comparison uses), so that the filter's colour weight tells an edge from noise.  The denoiser's defaults do not:
# sigmaColour 16 leaves the colour weight at 1 for every pair of colours in [0, 1], five passes then blur across shading the guides do
# not see, and the blur's own error (RMSE about 0.23 to 0.26 here, above the single frame's) hides what went in: with them "temporal
# denoised" and "frame denoised" agree to three digits.  Their figures are printed, not asserted.
QUALITY_DENOISE = dict(iterations=5, demodulate=0, sigmaColour=0.5, sigmaNormal=0.25, sigmaDepth=0.1)


def path_params(rtx, spp, mode):
    """(the params of the POSES poses, spheres, tris, infos)"""
    mgr = rtx.scenes.mesh_test_scene(QW, QH)
    params, spheres, tris, infos = mgr.build_buffers()
    params["numRaysPerPixel"], params["rngMode"] = spp, mode
    poses = [temporal_check.posed(rtx, mgr, params, np.multiply(PATH_STEP, i), PATH_YAW * i) for i in range(POSES)]
    return poses, spheres, tris, infos


@pytest.fixture(scope="module")
def converged_last(rtx, oracle):
    """the last pose, 8 frames of 128 samples per pixel (frame indices away from the path's)"""
    poses, s, t, m = path_params(rtx, 128, 1)
    image = None
    for k in range(8):                              # (the running mean starts at this render's first frame, whatever its frame index)
        cur = oracle.render_frame(poses[-1], s, t, m, 1000 + k, accel=True)[0]
        image = np.zeros_like(cur) if image is None else image
        oracle.accumulate(image, cur, k)
    image.setflags(write=False)
    return image


@pytest.fixture(scope="module")
def path_guides(rtx):
    """the feature planes of every pose (4 feature frames each; they do not depend on spp or rngMode beyond the sample count: 4 spp)"""
    poses, s, t, m = path_params(rtx, 4, 1)
    return [aov_check.oracle_planes(rtx, p, s, t, m, range(4)) for p in poses]


def run_path(rtx, oracle, guides, spp, mode, **kw):
    """(single frame at the last pose, plain accumulation over the path, T, the last pose's planes)"""
    poses, s, t, m = path_params(rtx, spp, mode)
    chk, accum = Checker(), None
    for i, p in enumerate(poses):
        cur = oracle.render_frame(p, s, t, m, i, accel=True)[0]
        frame = np.zeros_like(cur)
        oracle.accumulate(frame, cur, 0)                # resultTexture after rt_reset_accum and one frame
        accum = np.zeros_like(cur) if accum is None else accum
        oracle.accumulate(accum, cur, i)                # resultTexture when nobody resets it
        T, _ = chk.step(frame, *guides[i], p, **kw)
    return frame, accum, T, guides[-1]


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_temporal_image_beats_the_single_frame_and_plain_accumulation(rtx, oracle, converged_last, path_guides, spp, mode):
    frame, accum, T, (A, G) = run_path(rtx, oracle, path_guides, spp, mode, **temporal_check.DEFAULTS)
    r = {k: denoise_check.rmse(v, converged_last) for k, v in (("frame", frame), ("accumulated", accum), ("temporal", T))}
    for name, kw in (("denoised", QUALITY_DENOISE), ("denoised with the defaults", denoise_check.DEFAULTS)):
        r["frame " + name] = denoise_check.rmse(denoise_check.checker(frame, A, G, **kw), converged_last)
        r["temporal " + name] = denoise_check.rmse(denoise_check.checker(T, A, G, **kw), converged_last)
    print(f"{spp} spp, rngMode {mode}: RMSE " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert r["temporal"] < r["frame"]
    assert r["temporal"] < r["accumulated"]
    assert r["temporal denoised"] < r["frame denoised"]


# ---- (d) the boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)


def _c_fields(header, name):
    body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(?:const\s+)?\w+\s+", "", decl.strip())
        if decl:
            names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
    return names


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for cls in (rtx.Tracer, rtx.MultiTracer):
        for method in ("temporal", "reset_temporal", "read_temporal", "read_temporal_history", "read_temporal_display", "temporal_info",
                       "denoise_temporal"):
            assert hasattr(cls, method), (cls.__name__, method)
    assert hasattr(rtx.RayTracingManager, "Temporal")
    assert lib.rt_abi_version() == 1
    assert lib.rt_sizeof(b"rt_temporal_params") == 32 == rtx.TEMPORAL_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_temporal_info") == 32 == rtx.TEMPORAL_INFO.itemsize
    assert _c_fields(header, "rt_temporal_params") == list(rtx.TEMPORAL_PARAMS.names)
    assert _c_fields(header, "rt_temporal_info") == list(rtx.TEMPORAL_INFO.names)
    for key, macro in (("maxHistory", "MAX_HISTORY"), ("depthTolerance", "DEPTH_TOLERANCE"), ("normalTolerance", "NORMAL_TOLERANCE")):
        value = float(re.search(r"#define\s+RT_TEMPORAL_DEFAULT_" + macro + r"\s+([\d.]+)f?", header).group(1))
        assert value == rtx.TEMPORAL_DEFAULTS[key] == temporal_check.DEFAULTS[key], key


def test_csharp_and_cpp_hosts_carry_the_step():
    cs = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cs")
    native, backend = open(os.path.join(cs, "RtNative.cs")).read(), open(os.path.join(cs, "RtBackend.cs")).read()
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    for name in ("rt_temporal", "rt_reset_temporal", "rt_read_temporal", "rt_denoise_temporal", "rt_multi_temporal", "rt_multi_read_temporal",
                 "rt_multi_denoise_temporal"):
        assert name in used, name
    text = open(os.path.join(cs, "RtTemporal.cs")).read()
    structs = dict(re.findall(r"public\s+struct\s+(\w+)[^{]*\{(.*?)\n    \}", text, re.S))
    fields = {k: re.findall(r"public\s+(int|float|double)\s+([\w, ]+);", v) for k, v in structs.items()}
    flat = {k: [(t, n.strip()) for t, names in v for n in names.split(",")] for k, v in fields.items()}
    assert flat["RtTemporalParams"] == [("int", "maxHistory"), ("float", "depthTolerance"), ("float", "normalTolerance")] + \
        [("int", f"_reserved{i}") for i in range(5)]
    assert flat["RtTemporalInfo"] == [("int", "calls"), ("int", "width"), ("int", "height"), ("int", "_reserved"),
                                      ("double", "lastKernelMs"), ("double", "totalKernelMs")]
    hpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp", "rt_host.cpp")).read()
    assert re.search(r"\bTemporal\s*\(", hpp) and re.search(r"\brt_temporal\b", cpp) and re.search(r"\brt_multi_temporal\b", cpp)


def test_temporal_kernel_is_built_without_scratch_or_spilled_vgprs():
    found = set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            name = k[".name"]
            if "k_temporal" in name:
                found.add(name)
                assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (name, "scratch")
                assert "k_atrous" not in name and "k_denoise" not in name, name
                print(f"{name}: {k['.vgpr_count']} VGPRs, {k['.sgpr_count']} SGPRs")
    assert len(found) == 1, sorted(found)
