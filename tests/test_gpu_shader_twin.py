"""The HIP kernels against the float64 twin of the shader (tests/shader_twin.py), with the comparisons of tests/test_shader_twin_cpu.py:
ray queries through both BVH builders and the local-mesh path against brute force in double, rendered frames of both kernels, both random
streams, with and without camera-ray lists, and the feature buffers against what the twin finds along the frame's own camera rays.
Today the kernels equal the oracle bit for bit, so these pass when the CPU comparisons pass; they keep holding if a kernel is ever
allowed to leave bit parity.  Only tests/ and the product are used."""
import numpy as np
import pytest

import shader_twin as tw
import twin_cases as tc
from ray_query_helpers import camera_rays, scene_of

pytestmark = pytest.mark.gpu


def loaded(rtx, inputs, **options):
    params, spheres, tris, infos = inputs
    t = rtx.Tracer(0)
    for k, v in options.items():
        t.set_option(k, v)
    t.set_params(params)
    t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
    return t


def check_queries(t, geometry, mode, rays, key):
    twin = tw.closest_hit(tw.Scene(None, *geometry, mode=mode), rays)
    tc.check_hits(t.trace_rays(rays), twin, rays, key)
    firm = twin["margin"] >= tc.margin_threshold(key)
    occ = t.occluded(rays)
    assert np.array_equal(occ[firm] != 0, twin["kind"][firm] != 0), key + ": occlusion"
    return twin


@pytest.mark.parametrize("device_bvh", [0, 1])
@pytest.mark.parametrize("name, mode", [("Knight", 0), ("Reflective_Balls", 1), ("Suzanne", 0)])
def test_trace_rays_on_camera_rays(rtx, name, mode, device_bvh):
    params, spheres, tris, infos = scene_of(rtx, name).build_buffers()
    params["intersectMode"] = mode
    with loaded(rtx, (params, spheres, tris, infos), device_bvh=device_bvh) as t:
        twin = check_queries(t, (spheres, tris, infos), mode, camera_rays(rtx, params), f"camera/{name}/mode{mode}")
        assert (twin["kind"] != 0).sum() > 100


@pytest.mark.parametrize("device_bvh, mode", [(0, 0), (1, 1)])
def test_trace_rays_on_random_scaled_and_surface_rays(rtx, device_bvh, mode):
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(64, 48).build_buffers()
    params["intersectMode"] = mode
    geometry = (spheres, tris, infos)
    with loaded(rtx, (params, spheres, tris, infos), device_bvh=device_bvh) as t:
        first = None
        for label, rays in tc.random_ray_sets(rtx, spheres, tris, mode):
            twin = check_queries(t, geometry, mode, rays, f"random/{label}/mode{mode}")
            first = twin if first is None else first
        check_queries(t, geometry, mode, tc.surface_rays(rtx, first, spheres, tris), f"surface/mode{mode}")


def test_trace_rays_through_moved_local_meshes(rtx):
    """The device gets local meshes and, after a first frame, new poses; the twin gets the world triangles and chunk boxes that the host
    marshals for those poses, so a geometry pass that applied a pose wrongly would be seen."""
    before, moved, (params, spheres, tris, infos) = tc.moved_mesh_scene(rtx)
    ltris, chunks = before.build_local_buffers()
    with rtx.Tracer(0) as t:
        t.set_params(params)
        t.upload(spheres=spheres)
        t.upload_local_meshes(ltris, chunks, len(before.meshes))
        t.set_mesh_transforms(before.build_transforms())
        t.render(0, 1)
        t.set_mesh_transforms(moved)
        twin = check_queries(t, (spheres, tris, infos), 0, camera_rays(rtx, params), "camera_moved/mode0")
        assert (twin["kind"] == 2).sum() > 100
        world, winfos = t.read_world_geometry()                   # besides: the device's world geometry is the host's, byte for byte
        assert all(world[k].tobytes() == tris[k].tobytes() for k in tris.dtype.names)
        assert winfos["boundsMin"].tobytes() == infos["boundsMin"].tobytes() and winfos["boundsMax"].tobytes() == infos["boundsMax"].tobytes()


@pytest.mark.parametrize("primary_lists", [0, 1])
@pytest.mark.parametrize("rng_mode", [0, 1], ids=["pcg", "philox"])
@pytest.mark.parametrize("kernel", [0, 1])
def test_rendered_frames(rtx, kernel, rng_mode, primary_lists):
    for case in ("mesh_every_branch", "Knight", "environment_focus_500"):
        inputs = tc.frame_inputs(rtx, case, rng_mode)
        frame = tc.FRAME_CASES[case][1][-1]
        twin = tw.render_frame(tw.Scene(*inputs), frame)
        with loaded(rtx, inputs, kernel=kernel, primary_lists=primary_lists) as t:
            t.render(frame, 1)
            got = t.read_last_frame()
        tc.check_frame(got, twin, tc.frame_key(case, rng_mode, frame))


def test_feature_buffers_of_one_frame(rtx):
    """rt_render_aov against tw.feature_frame (the definition of include/rt.h read by the twin along the frame's own camera rays)"""
    inputs = tc.frame_inputs(rtx, tc.FEATURE_CASE, 1)
    twin = tw.feature_frame(tw.Scene(*inputs), tc.FEATURE_FRAME)
    with loaded(rtx, inputs) as t:
        t.render_aov(tc.FEATURE_FRAME, 1)
        got = np.concatenate([t.read_aov(rtx.RT_AOV_ALBEDO), t.read_aov(rtx.RT_AOV_NORMAL_DEPTH)], -1)
    tc.check_features(got, twin, f"aov/{tc.FEATURE_CASE}/frame{tc.FEATURE_FRAME}")
    assert (twin[0][..., 3] == 1).sum() > 100 and (twin[0][..., 3] == 0).any()
