"""The oracle against a float64 twin of the shader (tests/shader_twin.py): a second opinion on the float part of the path, which every
other test takes from oracle/rt_oracle.c alone.  The twin is written from the shader's text and draws the same random integers, so it
walks the oracle's light paths and the comparison is per ray and per pixel.  Tolerances, the fragile filter and its caps: tests/twin_cases.py.
The twin's own hits are checked geometrically in double, and deliberate misreadings of the shader, applied to the twin, must make the
comparison fail."""
import json
import os

import numpy as np
import pytest

import shader_twin as tw
import twin_cases as tc
from query_check import oracle_hits
from ray_query_helpers import GOLDEN, camera_rays, scene_of, shim      # noqa: F401 (shim is a fixture)


# ---- the twin's integer streams ------------------------------------------------------------------------------------------------------
def test_twin_pcg_matches_the_known_answers():
    kat = json.load(open(os.path.join(GOLDEN, "pcg_kat.json")))
    for seed, exp in kat.items():
        state, got = int(seed), []
        for _ in range(4):
            state, r = tw.pcg_next(state)
            got.append(r)
        assert got == exp["outputs"] and state == exp["state"], seed
    seeds = np.array([int(s) for s in kat], np.uint64)                       # the array form the twin renders with
    state, r = tw.pcg_next(seeds)
    assert r.tolist() == [kat[s]["outputs"][0] for s in kat]


def test_twin_philox_array_form_matches_the_integer_form():
    ctr, key = (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)
    want = tw.philox4x32_10(ctr, key)
    assert want == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    got = tw.philox4x32_10(tuple(np.array([c, 0], np.uint64) for c in ctr), tuple(np.array([k, 0], np.uint64) for k in key))
    assert tuple(int(g[0]) for g in got) == want and tuple(int(g[1]) for g in got) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


# ---- closest hit ---------------------------------------------------------------------------------------------------------------------
def assert_twin_hits_are_geometrically_right(geometry, rays, hits, threshold, what):
    """Independently of the oracle and of the twin's formulas, in double: the hit point lies on the triangle's plane and inside its edges
    (or on the sphere), and no primitive that a ray meets clearly (by more than the margin threshold) lies closer.  Planes are
    intersected directly and the inside test is three edge functions; spheres go through the closest approach to the centre."""
    spheres, tris, infos = geometry
    o, d = np.asarray(rays["origin"], np.float64), np.asarray(rays["direction"], np.float64)
    firm = hits["margin"] >= threshold
    A, B, C = (np.asarray(tris[k], np.float64).reshape(-1, 3) for k in ("posA", "posB", "posC"))
    centre, radius = np.asarray(spheres["position"], np.float64).reshape(-1, 3), np.asarray(spheres["radius"], np.float64).reshape(-1)
    used = np.concatenate([np.arange(f, f + c) for f, c in zip(infos["firstTriangleIndex"], infos["numTriangles"])] + [np.zeros(0, np.int64)]).astype(np.int64)
    P = o + d * np.where(hits["kind"] != 0, hits["dst"], 0.0)[:, None]
    size = np.maximum(np.abs(P).max(1), np.abs(o).max(1)) + 1.0
    with np.errstate(all="ignore"):
        t = np.nonzero(firm & (hits["kind"] == tw.RT_HIT_TRIANGLE))[0]
        a, b, c = A[hits["primitive"][t]], B[hits["primitive"][t]], C[hits["primitive"][t]]
        n = np.cross(b - a, c - a)
        n2 = np.sum(n * n, 1)
        assert (np.abs(np.sum((P[t] - a) * n, 1)) / np.sqrt(n2) <= 1e-9 * size[t]).all(), what + ": a hit point off its triangle's plane"
        for p0, p1 in ((a, b), (b, c), (c, a)):
            assert (np.sum(np.cross(p1 - p0, P[t] - p0) * n, 1) / n2 >= -1e-9).all(), what + ": a hit point outside its triangle"
        assert (np.sum(d[t] * n, 1) < 0).all() and (hits["dst"][t] >= 0).all(), what + ": a back face or a hit behind the origin"
        s = np.nonzero(firm & (hits["kind"] == tw.RT_HIT_SPHERE))[0]
        k = hits["primitive"][s]
        assert (np.abs(np.linalg.norm(P[s] - centre[k], axis=1) - radius[k]) <= 1e-9 * size[s]).all(), what + ": a hit point off its sphere"
        assert (np.sum(d[s] * (P[s] - centre[k]), 1) <= 0).all(), what + ": a sphere's far side"
        # nothing clearly valid closer (a miss: nothing clearly valid at all)
        limit = np.where(hits["kind"] != 0, hits["dst"] * (1 - threshold), np.inf)
        len_d = np.linalg.norm(d, axis=1)
        step = max(1, 400_000 // max(1, len(used)))
        a, b, c = A[used], B[used], C[used]
        n = np.cross(b - a, c - a)
        n2 = np.sum(n * n, 1)
        closer = np.zeros(len(o), bool)
        for i in range(0, len(o), step):
            oo, dd = o[i:i + step, None, :], d[i:i + step, None, :]
            denom = np.sum(dd * n[None], -1)
            tt = np.sum((a[None] - oo) * n[None], -1) / denom
            Q = oo + dd * tt[..., None]
            inside = np.ones(tt.shape, bool)
            for p0, p1 in ((a, b), (b, c), (c, a)):
                inside &= np.sum(np.cross((p1 - p0)[None], Q - p0[None]) * n[None], -1) / n2[None] > threshold
            front = -denom >= 1e-6 + threshold * len_d[i:i + step, None] * np.sqrt(n2)[None]
            ahead = tt * len_d[i:i + step, None] > threshold * np.linalg.norm(oo - a[None], axis=-1)
            closer[i:i + step] |= (inside & front & ahead & (tt < limit[i:i + step, None])).any(1)
            if len(radius):
                oc = oo - centre[None]
                along = -np.sum(oc * dd, -1) / len_d[i:i + step, None] ** 2
                off2 = np.sum((oc + dd * along[..., None]) ** 2, -1)
                half = np.sqrt((radius[None] ** 2 - off2)) / len_d[i:i + step, None]
                ts = along - half
                clear = (off2 < radius[None] ** 2 * (1 - threshold) ** 2) & (ts * len_d[i:i + step, None] > threshold * np.linalg.norm(oc, axis=-1))
                closer[i:i + step] |= (clear & (ts < limit[i:i + step, None])).any(1)
    bad = np.nonzero(firm & closer)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rays meet something clearly valid closer than the twin's hit, first {bad[:5].tolist()}"


def compare_oracle_hits(rtx, shim, key, geometry, mode, rays):
    twin = tw.closest_hit(tw.Scene(None, *geometry, mode=mode), rays)
    got = oracle_hits(rtx, shim, *geometry, mode, rays)
    observed = tc.check_hits(got, twin, rays, key)
    assert_twin_hits_are_geometrically_right(geometry, rays, twin, tc.margin_threshold(key), key)
    return twin, observed


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", tc.RAY_SCENES)
def test_oracle_closest_hit_on_camera_rays(rtx, shim, name, mode):
    params, spheres, tris, infos = scene_of(rtx, name).build_buffers()
    twin, _ = compare_oracle_hits(rtx, shim, f"camera/{name}/mode{mode}", (spheres, tris, infos), mode, camera_rays(rtx, params))
    assert (twin["kind"] != 0).sum() > 100


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_closest_hit_on_random_scaled_and_surface_rays(rtx, shim, mode):
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(64, 48).build_buffers()
    geometry = (spheres, tris, infos)
    first = None
    for label, rays in tc.random_ray_sets(rtx, spheres, tris, mode):
        twin, _ = compare_oracle_hits(rtx, shim, f"random/{label}/mode{mode}", geometry, mode, rays)
        first = twin if first is None else first
    assert (first["kind"] == 1).any() and (first["kind"] == 2).any() and (first["kind"] == 0).any()
    rays = tc.surface_rays(rtx, first, spheres, tris)
    twin, _ = compare_oracle_hits(rtx, shim, f"surface/mode{mode}", geometry, mode, rays)
    assert len(rays) > 400 and (twin["kind"] != 0).sum() > 50


def test_oracle_closest_hit_through_nan_chunk_boxes(rtx, shim):
    """RayBoundingBox :177-187 on chunk boxes with a NaN boundsMin component, a NaN boundsMax component and every face NaN (what the
    reference's marshal gives a chunk whose last vertex is NaN): the float64 twin's min / max skip a NaN operand as HLSL's
    do, and the oracle's loop cuts the same triangles off.  The NaN faces decide: with the finite boxes those chunks are hit."""
    key, geometry, mode, rays = tc.nan_box_case(rtx)
    twin = tw.closest_hit(tw.Scene(None, *geometry, mode=mode), rays)
    tc.check_hits(oracle_hits(rtx, shim, *geometry, mode, rays), twin, rays, key)     # (no geometric check: these boxes cut triangles off)
    spheres, tris, infos = geometry
    nan_chunks = np.nonzero(np.isnan(infos["boundsMin"]).any(1) | np.isnan(infos["boundsMax"]).any(1))[0]
    all_nan = np.nonzero(np.isnan(infos["boundsMin"]).all(1) & np.isnan(infos["boundsMax"]).all(1))[0]
    assert len(nan_chunks) == 3 and len(all_nan) == 1
    finite = rtx.scenes.mesh_test_scene(32, 24).build_buffers()[3]
    plain = tw.closest_hit(tw.Scene(None, spheres, tris, finite, mode=mode), rays)
    tri = tw.RT_HIT_TRIANGLE
    seen = [int(((plain["kind"] == tri) & (plain["chunk"] == c)).sum()) for c in nan_chunks]
    print("rays that end in the three chunks with their finite boxes:", seen, "and with the NaN faces:",
          [int(((twin["kind"] == tri) & (twin["chunk"] == c)).sum()) for c in nan_chunks])
    assert sum(seen) > 60 and ((plain["kind"] == tri) & (plain["chunk"] == all_nan[0])).sum() > 20, seen
    assert not ((twin["kind"] == tri) & (twin["chunk"] == all_nan[0])).any(), "a box of NaN faces let a ray through"
    moved = (twin["kind"] != plain["kind"]) | (twin["primitive"] != plain["primitive"])
    assert moved.sum() > 60


# ---- whole frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_mode", [0, 1], ids=["pcg", "philox"])
@pytest.mark.parametrize("case", list(tc.FRAME_CASES))
def test_oracle_frames(rtx, oracle, case, rng_mode):
    inputs = tc.frame_inputs(rtx, case, rng_mode)
    branches = set()
    for frame in tc.FRAME_CASES[case][1]:
        twin = tw.render_frame(tw.Scene(*inputs), frame)
        got, _ = oracle.render_frame(*inputs, frame)
        tc.check_frame(got, twin, tc.frame_key(case, rng_mode, frame))
        assert (got[..., 3] == 1).all()
        branches |= twin["branches"]
    if case == "mesh_every_branch":
        assert branches >= tc.EVERY_BRANCH, tc.EVERY_BRANCH - branches
    if case.startswith("environment"):
        assert branches == {"miss"}
        assert got[..., :3].max() > 2 * got[..., :3].min() > 0          # the sun and the ground are both in view
        # the pixel-centre rays reach the ground, both ramps of GetEnvironmentLight (:244-245), the plateau above them, and the sun
        sc = tw.Scene(*inputs)
        y = np.concatenate([tw.camera_rays(sc, 0, s)[1][:, 1] for s in range(2)])
        counts = [int(((lo <= y) & (y < hi)).sum()) for lo, hi in ((-1, -0.01), (-0.01, 0), (0, 0.4), (0.4, 1))]
        assert counts[0] > 500 and counts[1] >= 20 and counts[2] > 500 and counts[3] > 200, counts
        d = np.concatenate([tw.camera_rays(sc, 0, s)[1] for s in range(2)])
        assert (d @ sc.p["worldSpaceLightPos0"]).max() > 0.999


def test_environment_off_is_exactly_black(rtx, oracle):
    inputs = list(tc.frame_inputs(rtx, "environment_focus_1", 0))
    inputs[0]["environmentEnabled"] = 0
    twin = tw.render_frame(tw.Scene(*inputs), 0)
    got, _ = oracle.render_frame(*inputs, 0)
    assert (twin["image"][..., :3] == 0).all() and (got[..., :3] == 0).all() and (got[..., 3] == 1).all()


def test_crop_of_the_twin_is_the_window_of_its_frame(rtx):
    inputs = tc.frame_inputs(rtx, "mesh", 0)
    full = tw.render_frame(tw.Scene(*inputs), 1)["image"]
    crop = tw.render_frame(tw.Scene(*inputs), 1, rect=(10, 5, 20, 12))["image"]
    assert np.array_equal(crop, full[5:12, 10:20])


def test_oracle_feature_frame(rtx):
    """the feature buffers' checker (tests/aov_oracle.c, built on the oracle) against the twin's reading of rt_render_aov's definition"""
    import aov_check
    inputs = tc.frame_inputs(rtx, tc.FEATURE_CASE, 1)
    twin = tw.feature_frame(tw.Scene(*inputs), tc.FEATURE_FRAME)
    albedo, normal_depth = aov_check.oracle_frame(rtx, *inputs, tc.FEATURE_FRAME, accel=False)
    tc.check_features(np.concatenate([albedo, normal_depth], -1), twin, f"aov/{tc.FEATURE_CASE}/frame{tc.FEATURE_FRAME}")
    assert (twin[0][..., 3] == 1).sum() > 100 and (twin[0][..., 3] == 0).any()


def test_the_recorded_measurements_are_what_the_twins_give(rtx):
    """MEASURED is pasted from `python tests/twin_cases.py`; two fast rows are measured again so that the table cannot drift from the code"""
    for case, rng_mode, frame in (("environment_focus_1", 0, 0), ("Reflective_Balls", 1, 7)):
        _, err, margin, mean = tc.twin_pair_on_frame(tc.frame_inputs(rtx, case, rng_mode), frame)
        want = tc.MEASURED[tc.frame_key(case, rng_mode, frame)]
        assert err == pytest.approx(want[0], rel=2e-3) and mean == pytest.approx(want[2], rel=2e-3), (case, err, margin, mean, want)
        assert (margin is None) == (want[1] is None)


# ---- accumulate ------------------------------------------------------------------------------------------------------------------------
def test_oracle_accumulate(oracle):
    rng = np.random.default_rng(2)
    acc = np.zeros(64, np.float32)
    twin = acc.astype(np.float64)
    for frame in range(3):
        cur = (rng.random(64) * 1.5 - 0.2).astype(np.float32)                # below 0 and above 1 as well
        cur[frame] = np.nan
        oracle.accumulate(acc, cur, frame)
        twin = tw.accumulate(twin.astype(np.float32), cur, frame)
        assert not np.isnan(acc).any() and acc[frame] in (0.0, twin[frame].astype(np.float32))
        assert (np.abs(acc - twin) <= 4 * np.spacing(np.maximum(np.abs(twin), 1e-3).astype(np.float32))).all(), frame
        acc = twin.astype(np.float32)                                         # both continue from the same float32 texture


# ---- the comparison can fail ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misread, case", [("swap_uv", "mesh"), ("sun_ungated", "environment_focus_1"), ("swap_pi", "mesh_dof"),
                                           ("checker_xy", "mesh"), ("smooth_no_flag", "mesh"), ("emit_after", "mesh_every_branch")])
def test_a_misread_shader_fails_the_comparison(rtx, oracle, misread, case):
    """the same comparison with one deliberate misreading switched on in the twin: tolerances and the fragile filter still see it"""
    inputs = tc.frame_inputs(rtx, case, 0)
    frame = tc.FRAME_CASES[case][1][0]
    got, _ = oracle.render_frame(*inputs, frame)
    wrong = tw.render_frame(tw.Scene(*inputs, misread=(misread,)), frame)
    wrong["margin"] = tw.render_frame(tw.Scene(*inputs), frame)["margin"]       # the fragile set of the true reading: the filter hides nothing
    with pytest.raises(AssertionError, match="beyond|means differ"):
        tc.check_frame(got, wrong, tc.frame_key(case, 0, frame))


def test_a_misread_normal_fails_the_hit_comparison(rtx, shim):
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(64, 48).build_buffers()
    rays = camera_rays(rtx, params)
    got = oracle_hits(rtx, shim, spheres, tris, infos, 1, rays)
    wrong = tw.closest_hit(tw.Scene(None, spheres, tris, infos, mode=1, misread=("swap_uv",)), rays)
    with pytest.raises(AssertionError, match="rays differ"):
        tc.check_hits(got, wrong, rays, "camera/mesh_test_scene/mode1")
