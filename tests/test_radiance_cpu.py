"""Radiance queries without a GPU: the checker (tests/query_oracle.c, the oracle's own trace() per ray and sample) is pinned to the
renderer's oracle, to its tree restated in numpy and to analytic cases, and the ABI is declared, exported and bound.

1. rad_trace over rad_camera_rays with samples 1 and seed f is the rgb of orc_render_frame in Philox mode with numRaysPerPixel 1.
2. The tree: N per-sample values of one ray, re-added in numpy float32 by the written rule.
3. Analytic cases: an empty scene, an emitting sphere, tMax around the hit distance, rays that are not traced.
4. Split invariance under firstIndex.
5. Boundary: struct sizes, exports, layouts, methods, the kernels in the code object without scratch."""
import os
import re

import numpy as np
import pytest

import query_check as rc
from ray_query_helpers import camera_rays, make_rays, scene_of
from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_trace_radiance", "rt_trace_radiance_device", "rt_get_radiance_info", "rt_multi_trace_radiance")


def light_scene(rtx, width=64, height=48):
    """mesh_test_scene (two analytic spheres, cubes, tessellated spheres, a checker floor, an emissive quad) with every fourth object an
    InvisibleLight that emits"""
    mgr = rtx.scenes.mesh_test_scene(width, height)
    for i, mesh in enumerate(mgr.meshes[2:]):
        if i % 4 == 0:
            for mat in mesh.materials:
                mat.flag = rtx.MaterialFlag.InvisibleLight
                mat.emissionColour, mat.emissionStrength = (1.0, 0.8, 0.6, 1.0), 2.0
    params, spheres, tris, infos = mgr.build_buffers()
    assert (infos["material"]["flag"] == 2).any() and len(spheres) > 0
    return params, spheres, tris, infos


def reference_scene(rtx, width=64, height=48):
    from rtx_amd import unity_scene
    mgr = unity_scene.load_scene_npz(os.path.join(ROOT, "tests", "golden", "scenes", "Reflective_Balls.npz"), width, height)
    params, spheres, tris, infos = mgr.build_buffers()
    assert len(spheres) > 0 and len(tris) > 0
    return params, spheres, tris, infos


@pytest.mark.parametrize("bounces", [0, 1, 8])
@pytest.mark.parametrize("size, defocus", [((64, 48), 0.0), ((16, 12), 30.0)])
@pytest.mark.parametrize("scene", [light_scene, reference_scene])
def test_checker_equals_the_philox_frame_of_the_oracle(rtx, oracle, scene, size, defocus, bounces):
    params, spheres, tris, infos = scene(rtx, *size)
    params["maxBounceCount"], params["numRaysPerPixel"], params["rngMode"] = bounces, 1, 1
    params["defocusStrength"] = defocus
    frame = 5
    image, _ = oracle.render_frame(params, spheres, tris, infos, frame, accel=True)
    rays = rc.frame_camera_rays(rtx, params, frame)
    if defocus:
        assert len(np.unique(rays["origin"], axis=0)) > len(rays) // 2
    got = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 1, seed=frame)
    rc.assert_same_bits(got, image.reshape(-1, 4), f"{scene.__name__} {size} bounces {bounces}")
    assert (got[:, 3] == 1).all() and len(np.unique(got[:, :3], axis=0)) > 1                # (not a constant image)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 21, 64])
def test_the_tree_is_the_written_rule(rtx, n):
    params, spheres, tris, infos = light_scene(rtx)
    params["maxBounceCount"] = 4
    rays = camera_rays(rtx, params)[[64 * 10 + 20, 64 * 24 + 32, 64 * 40 + 50]]
    seed, first = 9, 1000
    got = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, n, seed=seed, first_index=first)
    varied = False
    for i in range(len(rays)):
        values = np.stack([rc.oracle_radiance_sample(rtx, params, spheres, tris, infos, rays[i:i + 1], s, seed=seed, index=first + i) for s in range(n)])
        varied = varied or len(np.unique(values, axis=0)) > 1
        rc.assert_same_bits(got[i, :3], rc.tree_sum(values), f"N = {n}, ray {i}")
        assert got[i, 3] == 1
    assert varied or n == 1


def empty_scene(rtx, width=16, height=12):
    cam = rtx.Camera(rtx.Transform(position=(0.0, 1.0, -5.0), rotation=(-0.2, 0.1, 0.0, 0.97)), fieldOfView=70.0, aspect=width / height)
    mgr = rtx.RayTracingManager(cam, rtx.Light(rtx.scenes.BALLS_OUTDOORS_LIGHT), width, height)
    mgr.maxBounceCount, mgr.numRaysPerPixel, mgr.divergeStrength, mgr.defocusStrength = 3, 1, 0.0, 0.0
    mgr.environmentSettings = rtx.EnvironmentSettings(**rtx.scenes.BALLS_OUTDOORS_ENV)
    return mgr


@pytest.mark.parametrize("n", [1, 2, 4, 16, 64])
def test_an_empty_scene_gives_the_environment_term(rtx, oracle, n):
    params, spheres, tris, infos = empty_scene(rtx).build_buffers()
    assert params["environmentEnabled"] == 1
    params["rngMode"] = 1
    sky, _ = oracle.render_frame(params, spheres, tris, infos, 0)            # one miss per pixel: GetEnvironmentLight of the camera ray
    rays = rc.frame_camera_rays(rtx, params, 0)
    got = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, n, seed=3, first_index=77)
    rc.assert_same_bits(got, sky.reshape(-1, 4), f"N = {n}")
    assert len(np.unique(got[:, :3], axis=0)) > 4 and (got[:, :3] > 0).any()


def emitting_sphere(rtx):
    mgr = empty_scene(rtx)
    mgr.spheres.append(rtx.RayTracedSphere(rtx.Transform(position=(0.0, 0.0, 0.0), lossyScale=(2.0, 2.0, 2.0)),
                                           rtx.RayTracingMaterial(colour=(0.0, 0.0, 0.0, 1.0), emissionColour=(0.25, 0.25, 0.25, 1.0), emissionStrength=2.0,
                                                                  specularProbability=0.0)))
    params, spheres, tris, infos = mgr.build_buffers()
    spheres["material"]["emissionColour"] = (0.25, 0.25, 0.25, 1.0)          # (as given: no colour-space conversion)
    assert spheres["radius"][0] == 1.0
    return params, spheres, tris, infos


def test_an_emitting_black_sphere_gives_its_emission(rtx):
    params, spheres, tris, infos = emitting_sphere(rtx)
    rays = make_rays(rtx, [(0.0, 0.0, -5.0), (0.3, 0.2, -4.0)], [(0.0, 0.0, 1.0), (0.0, 0.0, 2.0)])
    got = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 16)
    assert got.tolist() == [[0.5, 0.5, 0.5, 1.0]] * 2


def test_tmax_around_the_hit_distance_flips_between_surface_and_sky(rtx):
    params, spheres, tris, infos = emitting_sphere(rtx)
    o, d = [(0.0, 0.0, -5.0)] * 5, [(0.0, 0.0, 1.0)] * 5                     # the hit is at dst = 4 exactly
    four = np.float32(4.0)
    t = np.array([np.nextafter(four, np.float32(0)), four, np.nextafter(four, np.float32(np.inf)), np.inf, 100.0], np.float32)
    got = rc.oracle_radiance(rtx, params, spheres, tris, infos, make_rays(rtx, o, d, t), 4)
    sky = rc.oracle_radiance(rtx, params, spheres[:0], tris, infos, make_rays(rtx, o[:1], d[:1]), 4)[0]
    assert sky.tolist() != [0.5, 0.5, 0.5, 1.0]
    for i in (0, 1):                                                         # dst < tMax fails: the sky's answer
        rc.assert_same_bits(got[i], sky, f"tMax {t[i]!r}")
    for i in (2, 3, 4):
        assert got[i].tolist() == [0.5, 0.5, 0.5, 1.0], t[i]


def test_rays_with_no_positive_tmax_are_not_traced(rtx):
    params, spheres, tris, infos = emitting_sphere(rtx)
    t = np.array([0.0, -0.0, -1.0, np.nan, -np.inf], np.float32)
    rays = make_rays(rtx, [(0.0, 0.0, -5.0)] * 5, [(0.0, 0.0, 1.0)] * 5, t)
    got, casts = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 16, count_casts=True)
    assert (got.view(np.uint32) == 0).all() and casts == 0


def test_the_checker_is_split_invariant_under_first_index(rtx):
    params, spheres, tris, infos = light_scene(rtx)
    rays = camera_rays(rtx, params)[::7][:200]
    whole = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 5, seed=2, first_index=0xFFFFFF80)      # (the index wraps inside the batch)
    for cut in (1, 77, 128, 199):
        a = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays[:cut], 5, seed=2, first_index=0xFFFFFF80)
        b = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays[cut:], 5, seed=2, first_index=0xFFFFFF80 + cut)
        rc.assert_same_bits(np.concatenate([a, b]), whole, f"cut at {cut}")
    other = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 5, seed=2, first_index=1)
    assert (other != whole).any()


def test_the_search_tree_does_not_change_the_checker(rtx):
    params, spheres, tris, infos = scene_of(rtx, "Knight").build_buffers()
    rays = camera_rays(rtx, params)[::5]
    a = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 3, accel=True)
    b = rc.oracle_radiance(rtx, params, spheres, tris, infos, rays, 3, accel=False)
    rc.assert_same_bits(a, b, "tree against loop")


# ---- 5. boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for cls in (rtx.Tracer, rtx.MultiTracer):
        assert hasattr(cls, "trace_radiance")
    assert hasattr(rtx.Tracer, "radiance_info")
    assert hasattr(rtx.RayTracingManager, "TraceRadiance") and hasattr(rtx.RayTracingManager, "TraceRadianceTensor")
    assert hasattr(rtx.host_cpp_binding.CppScene, "trace_radiance")
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    assert lib.rt_sizeof(b"rt_radiance_params") == 32 == rtx.RADIANCE_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_radiance_info") == 32 == rtx.RADIANCE_INFO.itemsize
    header = _header()
    for name, dt in (("rt_radiance_params", rtx.RADIANCE_PARAMS), ("rt_radiance_info", rtx.RADIANCE_INFO)):
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)


def test_csharp_radiance_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtRadiance.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtRadianceParams": ("rt_radiance_params", rtx.RADIANCE_PARAMS), "RtRadianceInfo": ("rt_radiance_info", rtx.RADIANCE_INFO)}
    assert set(structs) == set(pairs)
    for cs_name, (c_name, dt) in pairs.items():
        rows, size, _ = _layout(structs, cs_name)
        assert size == lib.rt_sizeof(c_name.encode()) == dt.itemsize, (cs_name, size)
        assert [r[0] for r in rows] == list(dt.names), (cs_name, rows)
        for field, off, nbytes in rows:
            assert off == dt.fields[field][1] and nbytes == dt.fields[field][0].itemsize, (cs_name, field, off, nbytes)


def test_csharp_backend_and_compiled_host_reach_the_entry_points():
    native, backend = open(os.path.join(CS, "RtNative.cs")).read(), open(os.path.join(CS, "RtBackend.cs")).read()
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    assert {"rt_trace_radiance", "rt_multi_trace_radiance"} <= used
    assert re.search(r"public\s+float\[\]\s+TraceRadiance\s*\(\s*RtRay\[\]\s+rays", backend)
    for name in ("rt_radiance_params", "rt_radiance_info"):
        assert '"' + name + '"' in native, name                               # VerifyLayout
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "TraceRadiance(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    assert "rth_trace_radiance" in open(os.path.join(host, "rt_host_c.cpp")).read()


def test_radiance_kernels_are_built_without_scratch():
    names = set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_radiance" not in k[".name"]:
                continue
            names.add(k[".name"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (k[".name"], "scratch")
    assert len(names) == 2, sorted(names)           # f16 / f32 nodes
