"""Gather queries without a GPU: the checker (tests/query_oracle.c: the oracle's own random_direction() and trace() per point and sample)
is pinned to the oracle's Philox words and intrinsics, to the radiance checker, to its tree and basis restated in numpy and to analytic
cases, and the ABI is declared, exported and bound.

Two scenes are not the ones the feature request words.  It asks for a point "inside one emitting sphere" and for an "enclosing sphere":
RaySphere (RayTracing.shader:120-147) keeps the near root only and wants dst >= 0, so a ray that starts inside a sphere never hits it.
The enclosing emitter here is a box of one-sided triangles that face inwards, which every ray from inside hits.  And the constant-
radiance SH9 case picks its emission so that every per-sample term L * Y0 is a power of two: then every partial sum of the fixed tree is
exact and the 4 ulp the request allows cover the roundings of c_0 = ((L * Y0) / N) * 4 pi alone.  For an emission with a full mantissa
the tree's own rounding is larger than that whatever the code does — a sub-stream adds one value 256 times and rounds the same way
each time inside a binade: restated in numpy, N = 4096 gives -23 ulp for L = 0.5 and 1.0, -15 ulp for 0.75 and 1.5 — so that case
would test float32 addition, not the basis or the scale."""
import os
import re

import numpy as np
import pytest

import query_check as gc
import query_check as rc
from query_check import oracle_hits
from ray_query_helpers import camera_rays, make_rays, scene_of, shim  # noqa: F401  (shim: a fixture)
from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata
from test_radiance_cpu import empty_scene, light_scene

EXPORTS = ("rt_gather", "rt_gather_device", "rt_get_gather_info", "rt_multi_gather")
MODES = (gc.COSINE, gc.SH9)
f32 = np.float32


def surface_points(rtx, shim, params, spheres, tris, infos, rays):  # noqa: F811
    return gc.surface_points(rtx, oracle_hits(rtx, shim, spheres, tris, infos, int(params["intersectMode"]), rays))


# ---- 1. the direction draw ----------------------------------------------------------------------------------------------------
def numpy_random_direction(oracle, key, seed, sample):
    """RandomDirection (RayTracing.shader:207-223) from words 0..3 of block 0xFFFFFFFE and words 0, 1 of block 0xFFFFFFFF"""
    import ctypes
    L = oracle.lib
    L.orc_philox4x32_10.restype = None
    L.orc_philox4x32_10.argtypes = [ctypes.POINTER(ctypes.c_uint32)] * 3
    words = []
    for block in (0xFFFFFFFE, 0xFFFFFFFF):
        c, k, o = (ctypes.c_uint32 * 4)(block, sample, 0, 0), (ctypes.c_uint32 * 2)(key, seed), (ctypes.c_uint32 * 4)()
        L.orc_philox4x32_10(c, k, o)
        words += list(o)
    u = [f32(np.uint32(w)) * f32(2.3283064365386963e-10) for w in words[:6]]
    two_pi = f32(2.0) * f32(3.1415926)
    v = []
    for a, b in ((u[0], u[1]), (u[2], u[3]), (u[4], u[5])):
        theta = two_pi * a
        rho = np.sqrt(f32(-2.0) * f32(L.om_log(float(b))))
        v.append(f32(rho) * f32(L.om_cos(float(theta))))
    return normalize(np.array(v, f32))


def normalize(v):
    length = np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])))
    return np.array([v[0] / length, v[1] / length, v[2] / length], f32)


@pytest.mark.parametrize("key, seed, sample", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (12345, 678, 9), (0xFFFFFFFF, 0xFFFFFFFF, 65535)])
def test_direction_is_the_oracles_random_direction_on_the_written_blocks(rtx, oracle, key, seed, sample):
    want = numpy_random_direction(oracle, key, seed, sample)
    assert abs(float(np.linalg.norm(want.astype(np.float64))) - 1.0) < 1e-6
    for normal in ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (np.nan, 5.0, -2.0)):          # SH9 ignores the normal
        gc.assert_same_bits(gc.direction(normal, sample, seed, key, gc.SH9), want, f"SH9 ({key}, {seed}, {sample})")
    # n = 0: normalize(0 + R)
    gc.assert_same_bits(gc.direction((0.0, 0.0, 0.0), sample, seed, key, gc.COSINE), normalize(want), "COSINE, n = 0")
    n = np.array([0.6, 0.0, -0.8], f32)
    gc.assert_same_bits(gc.direction(n, sample, seed, key, gc.COSINE), normalize((n + want).astype(f32)), "COSINE, unit n")
    assert float(np.dot(gc.direction(n, sample, seed, key, gc.COSINE).astype(np.float64), n.astype(np.float64))) >= 0.0


def test_directions_differ_by_key_seed_and_sample_and_fill_their_lobes(rtx):
    base = gc.direction((0, 0, 0), 0, 0, 0, gc.SH9)
    for args in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert (gc.direction((0, 0, 0), *args, gc.SH9) != base).any(), args
    up = np.array([0.0, 1.0, 0.0], f32)
    sphere = np.stack([gc.direction(up, s, 4, 2, gc.SH9) for s in range(2000)]).astype(np.float64)
    lobe = np.stack([gc.direction(up, s, 4, 2, gc.COSINE) for s in range(2000)]).astype(np.float64)
    assert np.abs(sphere.mean(0)).max() < 6 * np.sqrt(1 / 3 / 2000)                  # uniform: mean 0, Var = 1/3 per axis
    assert (lobe[:, 1] >= 0).all() and abs(lobe[:, 1].mean() - 2 / 3) < 6 * np.sqrt(1 / 18 / 2000)      # cosine lobe: E cos = 2/3, Var = 1/18


# ---- 2. a sample is the radiance checker's sample along the drawn direction ------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bounces", [0, 1, 8])
def test_sample_equals_the_radiance_checkers_sample_along_the_direction(rtx, shim, mode, bounces):  # noqa: F811
    params, spheres, tris, infos = light_scene(rtx)
    params["maxBounceCount"] = bounces
    pts = surface_points(rtx, shim, params, spheres, tris, infos, camera_rays(rtx, params)[5::97])
    pts["tMax"][1::3] = f32(2.5)                                                     # a bound that rejects some first hits
    seed, first = 9, 1000
    differ = 0
    for i in range(len(pts)):
        for s in (0, 1, 7):
            d = gc.direction(pts["direction"][i], s, seed, first + i, mode)
            ray = make_rays(rtx, [pts["origin"][i]], [d], pts["tMax"][i])
            want = rc.oracle_radiance_sample(rtx, params, spheres, tris, infos, ray, s, seed=seed, index=first + i)
            got = gc.oracle_gather_sample(rtx, params, spheres, tris, infos, pts[i:i + 1], s, seed=seed, index=first + i, mode=mode)
            gc.assert_same_bits(got, want, f"point {i} sample {s}")
            unbounded = make_rays(rtx, [pts["origin"][i]], [d])
            differ += int((rc.oracle_radiance_sample(rtx, params, spheres, tris, infos, unbounded, s, seed=seed, index=first + i) != want).any())
    assert differ > 0                                                                # (the bound changed some samples)


# ---- 3. the tree and the basis ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 16, 17, 64])
def test_the_tree_is_the_written_rule(rtx, shim, n):  # noqa: F811
    params, spheres, tris, infos = light_scene(rtx)
    params["maxBounceCount"] = 4
    pts = surface_points(rtx, shim, params, spheres, tris, infos, camera_rays(rtx, params)[[64 * 10 + 20, 64 * 24 + 32, 64 * 40 + 50]])
    seed, first = 9, 1000
    for mode in MODES:
        got = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, n, seed, first, mode)
        varied = False
        for i in range(len(pts)):
            L = np.stack([gc.oracle_gather_sample(rtx, params, spheres, tris, infos, pts[i:i + 1], s, seed, first + i, mode) for s in range(n)])
            varied = varied or len(np.unique(L, axis=0)) > 1
            if mode == gc.COSINE:
                gc.assert_same_bits(got[i, :3], gc.tree_sum(L), f"N = {n}, point {i}")
                assert got[i, 3] == 1
            else:
                Y = np.stack([gc.sh_basis(gc.direction(pts["direction"][i], s, seed, first + i, mode)) for s in range(n)])     # (N, 9)
                terms = (L[:, None, :] * Y[:, :, None]).astype(f32)                 # (N, 9, 3): L_s.c * Y_k, one rounding each
                want = (gc.tree_sum(terms) * f32(12.566371)).astype(f32)
                gc.assert_same_bits(got[i, :, :3], want, f"SH9 N = {n}, point {i}")
                assert got[i, :, 3].tolist() == [1.0] + [0.0] * 8
        assert varied or n == 1


# ---- 4 - 6. analytic cases ------------------------------------------------------------------------------------------------------
def material(rtx, emission, strength):
    m = np.zeros((), rtx.MATERIAL)                                                   # colour 0, specular colour 0: a path ends at its first hit
    m["emissionColour"][:3], m["emissionColour"][3], m["emissionStrength"] = emission, 1.0, strength
    return m


def triangle_scene(rtx, corners, emission, strength, environment):
    """an empty scene's params with one chunk of flat triangles (A, B, C rows; the geometric normal as every vertex normal)"""
    params, spheres, _, _ = empty_scene(rtx).build_buffers()
    params["environmentEnabled"] = 1 if environment else 0
    params["intersectMode"] = 0
    c = np.asarray(corners, f32).reshape(-1, 3, 3)
    tris = np.zeros(len(c), rtx.TRIANGLE)
    tris["posA"], tris["posB"], tris["posC"] = c[:, 0], c[:, 1], c[:, 2]
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    tris["normalA"] = tris["normalB"] = tris["normalC"] = n
    infos = np.zeros(1, rtx.MESHINFO)
    infos["numTriangles"] = len(c)
    infos["material"] = material(rtx, emission, strength)
    infos["boundsMin"], infos["boundsMax"] = c.reshape(-1, 3).min(0), c.reshape(-1, 3).max(0)
    return params, spheres[:0], tris, infos


def inward_box(rtx, half, emission, strength, environment=False):
    """a box [-half, half]^3 about the origin whose twelve triangles face inwards: every ray from inside hits it"""
    h = float(half)
    corners = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            def p(a, b):
                q = [0.0, 0.0, 0.0]
                q[axis], q[u], q[v] = sign * h, a * h, b * h
                return q
            quad = [p(-1, -1), p(1, -1), p(1, 1), p(-1, 1)]
            if sign < 0:
                quad.reverse()                                                      # cross(B - A, C - A) points to the centre on both faces
            corners += [[quad[0], quad[2], quad[1]], [quad[0], quad[3], quad[2]]]
    scene = triangle_scene(rtx, corners, emission, strength, environment)
    t = scene[2]
    n = np.cross(t["posB"] - t["posA"], t["posC"] - t["posA"])
    assert (np.einsum("ij,ij->i", n, -t["posA"]) > 0).all()                          # every triangle faces the centre
    return scene


def point(rtx, origin, normal, t_max=np.inf):
    return make_rays(rtx, [origin], [normal], t_max)


def test_constant_radiance_inside_an_emitter(rtx):
    N = 4096
    e, k = (0.25, 0.5, 0.75), 2.0                                                    # e * k = 0.5, 1, 1.5: every sum up to N of them is exact
    scene = inward_box(rtx, 2.0, e, k)
    pt = point(rtx, (0.3, -0.2, 0.1), (0.0, 0.0, 1.0))
    got = gc.oracle_gather(rtx, *scene, pt, N, seed=5, mode=gc.COSINE)
    assert got.tolist() == [[0.5, 1.0, 1.5, 1.0]]
    for s in (0, 1, 4095):
        assert gc.oracle_gather_sample(rtx, *scene, pt, s, seed=5, mode=gc.SH9).tolist() == [0.5, 1.0, 1.5]

    # SH9: L with L * Y0 = 1/4 exactly in float32 (see the module docstring), two more channels by exact halving and doubling
    Y0 = f32(0.28209479)
    L = f32(0.25) / Y0
    L = next(c for c in (L, np.nextafter(L, f32(0)), np.nextafter(L, f32(2))) if f32(c * Y0) == f32(0.25))
    e = np.array([L, L * f32(0.5), L * f32(2.0)], f32)
    scene = inward_box(rtx, 2.0, e, 1.0)
    sh = gc.oracle_gather(rtx, *scene, pt, N, seed=5, mode=gc.SH9)[0]
    want0 = (e.astype(np.float64) * float(Y0)) * 4 * np.pi                            # c_0 = (e k Y0) 4 pi
    ulp = np.spacing(want0.astype(f32)).astype(np.float64)
    assert (np.abs(sh[0, :3].astype(np.float64) - want0) <= 4 * ulp).all(), (sh[0], want0)
    assert sh[:, 3].tolist() == [1.0] + [0.0] * 8
    bound = 6.0 * e.astype(np.float64) * np.sqrt(4 * np.pi / N)                       # six standard deviations: Var Y_k = 1 / (4 pi)
    assert (np.abs(sh[1:, :3].astype(np.float64)) <= bound).all(), (sh[1:], bound)
    assert (sh[1:, :3] != 0).all()


def test_a_one_sided_floor_tells_the_hemispheres_apart(rtx):
    e, k = (0.25, 0.5, 0.75), 2.0
    w = 1.0e4                                                                        # far larger than the point's height
    floor = [[(-w, 0, -w), (-w, 0, w), (w, 0, w)], [(-w, 0, -w), (w, 0, w), (w, 0, -w)]]
    scene = triangle_scene(rtx, floor, e, k, environment=False)
    assert (scene[2]["normalA"] == (0, 1, 0)).all()                                  # it faces up: only rays going down hit it
    above = (0.5, 1.0, -0.25)
    up = gc.oracle_gather(rtx, *scene, point(rtx, above, (0, 1, 0)), 64, seed=1)
    down = gc.oracle_gather(rtx, *scene, point(rtx, above, (0, -1, 0)), 64, seed=1)
    assert up.tolist() == [[0.0, 0.0, 0.0, 1.0]]
    assert down.tolist() == [[0.5, 1.0, 1.5, 1.0]]
    both = gc.oracle_gather(rtx, *scene, point(rtx, above, (0, 0, 0)), 4096, seed=1)[0]      # n = 0: the sphere, half of it sees the floor
    assert abs(float(both[0]) - 0.25) < 6 * 0.5 * np.sqrt(0.25 / 4096)


def test_tmax_around_the_hit_distance_flips_every_sample(rtx, shim):  # noqa: F811
    e, k = (0.25, 0.5, 0.75), 2.0
    scene = inward_box(rtx, 2.0, e, k, environment=True)
    params, spheres, tris, infos = scene
    o = (0.3, -0.2, 0.1)
    inside = [0.5, 1.0, 1.5, 1.0]
    # one bound for all samples: below the nearest wall every sample sees the sky, beyond the farthest corner every sample the wall
    near, far = f32(2.0 - 0.3), f32(np.sqrt(3.0) * 2.3)
    for mode in MODES:
        sky = gc.oracle_gather(rtx, params, spheres, tris[:0], infos[:0], point(rtx, o, (0, 1, 0)), 16, seed=2, mode=mode)
        lo = gc.oracle_gather(rtx, *scene, point(rtx, o, (0, 1, 0), np.nextafter(near, f32(0))), 16, seed=2, mode=mode)
        hi = gc.oracle_gather(rtx, *scene, point(rtx, o, (0, 1, 0), far), 16, seed=2, mode=mode)
        free = gc.oracle_gather(rtx, *scene, point(rtx, o, (0, 1, 0)), 16, seed=2, mode=mode)
        gc.assert_same_bits(lo, sky, f"mode {mode}: tMax below the nearest wall")
        gc.assert_same_bits(hi, free, f"mode {mode}: tMax beyond the farthest corner")
        assert (sky != free).any()
    # one sample per point, the bound at that sample's own hit distance: dst < tMax fails at tMax = dst and holds one ulp above
    n = 40
    pts = make_rays(rtx, [o] * n, [(0, 1, 0)] * n)
    d = gc.directions(rtx, pts, 0, seed=3, first_index=50)
    dst = oracle_hits(rtx, shim, spheres, tris, infos, 0, make_rays(rtx, [o] * n, d))["dst"]
    assert np.isfinite(dst).all() and len(np.unique(dst)) > n // 2
    sky1 = gc.oracle_gather(rtx, params, spheres, tris[:0], infos[:0], pts, 1, seed=3, first_index=50)
    for t_max, want in ((np.nextafter(dst, f32(0)), sky1), (dst, sky1), (np.nextafter(dst, f32(np.inf)), np.array([inside] * n, f32))):
        pts["tMax"] = t_max
        gc.assert_same_bits(gc.oracle_gather(rtx, *scene, pts, 1, seed=3, first_index=50), want, "per-sample bound")
    assert (sky1[:, :3] != np.array(inside[:3], f32)).any(1).all()


# ---- 7 - 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_points_with_no_positive_tmax_are_not_traced(rtx, mode):
    scene = inward_box(rtx, 2.0, (0.25, 0.5, 0.75), 2.0)
    t = np.array([0.0, -0.0, -1.0, np.nan, -np.inf], f32)
    pts = make_rays(rtx, [(0.0, 0.0, 0.0)] * 5, [(0.0, 1.0, 0.0)] * 5, t)
    got, casts = gc.oracle_gather(rtx, *scene, pts, 16, mode=mode, count_casts=True)
    assert (got.view(np.uint32) == 0).all() and casts == 0
    pts["tMax"][2] = 1.0e3
    got, casts = gc.oracle_gather(rtx, *scene, pts, 16, mode=mode, count_casts=True)
    assert casts == 16 and (got[2] != 0).any() and (np.delete(got, 2, 0).view(np.uint32) == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_the_checker_is_split_invariant_under_first_index(rtx, shim, mode):  # noqa: F811
    params, spheres, tris, infos = light_scene(rtx)
    pts = surface_points(rtx, shim, params, spheres, tris, infos, camera_rays(rtx, params)[::7][:200])
    first = 0xFFFFFF80                                                               # (the index wraps inside the batch)
    whole = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, 5, 2, first, mode)
    for cut in (1, 77, 128, 199):
        a = gc.oracle_gather(rtx, params, spheres, tris, infos, pts[:cut], 5, 2, first, mode)
        b = gc.oracle_gather(rtx, params, spheres, tris, infos, pts[cut:], 5, 2, first + cut, mode)
        gc.assert_same_bits(np.concatenate([a, b]), whole, f"cut at {cut}")
    other = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, 5, 2, 1, mode)
    assert (other != whole).any()
    assert (gc.oracle_gather(rtx, params, spheres, tris, infos, pts, 5, 3, first, mode) != whole).any()      # the seed


def test_the_search_tree_does_not_change_the_checker(rtx, shim):  # noqa: F811
    params, spheres, tris, infos = scene_of(rtx, "Knight").build_buffers()
    pts = surface_points(rtx, shim, params, spheres, tris, infos, camera_rays(rtx, params)[::16])
    for mode in MODES:
        a = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, 2, mode=mode, accel=True)
        b = gc.oracle_gather(rtx, params, spheres, tris, infos, pts, 2, mode=mode, accel=False)
        gc.assert_same_bits(a, b, f"tree against loop, mode {mode}")


# ---- 10. boundary -----------------------------------------------------------------------------------------------------------------
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
        assert hasattr(cls, "gather")
    assert hasattr(rtx.Tracer, "gather_info")
    assert hasattr(rtx.RayTracingManager, "Gather")
    assert hasattr(rtx.host_cpp_binding.CppScene, "gather")
    assert re.search(r"RT_GATHER_COSINE\s*=\s*0\s*,\s*RT_GATHER_SH9\s*=\s*1", header)
    assert (rtx.GATHER_COSINE, rtx.GATHER_SH9) == (0, 1)
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    assert lib.rt_sizeof(b"rt_gather_params") == 32 == rtx.GATHER_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_gather_info") == 32 == rtx.GATHER_INFO.itemsize
    header = _header()
    for name, dt in (("rt_gather_params", rtx.GATHER_PARAMS), ("rt_gather_info", rtx.GATHER_INFO)):
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)
    assert rtx.GATHER_PARAMS.names == ("samples", "seed", "firstIndex", "mode", "_reserved")
    assert rtx.GATHER_INFO.names == ("samples", "lastSampleLanes", "calls", "mode", "lastKernelMs", "totalKernelMs")


def test_csharp_gather_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtGather.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtGatherParams": ("rt_gather_params", rtx.GATHER_PARAMS), "RtGatherInfo": ("rt_gather_info", rtx.GATHER_INFO)}
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
    assert {"rt_gather", "rt_multi_gather"} <= used
    assert re.search(r"public\s+float\[\]\s+Gather\s*\(\s*RtRay\[\]\s+points", backend)
    for name in ("rt_gather_params", "rt_gather_info"):
        assert '"' + name + '"' in native, name                               # VerifyLayout
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "Gather(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    assert "rth_gather" in open(os.path.join(host, "rt_host_c.cpp")).read()


def _cs_method_body(source, signature):
    """the text between the braces of the method whose declaration matches `signature`"""
    m = re.search(signature, source)
    assert m, signature
    start = source.index("{", m.end())
    depth, i = 0, start
    while True:
        depth += {"{": 1, "}": -1}.get(source[i], 0)
        if depth == 0:
            return source[start + 1:i]
        i += 1


def test_csharp_gather_uses_no_local_before_its_declaration():
    """A C# local is in scope for its whole block: a name read above the line that declares it as a local binds to that local (CS0841),
    not to a field of the same name.  Nothing here compiles C#, so the text is checked: in RtBackend.Gather every local's first
    appearance is its declaration, and the default sample count is read from the RtParams field."""
    backend = open(os.path.join(CS, "RtBackend.cs")).read()
    body = re.sub(r"//[^\n]*", "", _cs_method_body(backend, r"public\s+float\[\]\s+Gather\s*\("))
    locals_ = re.findall(r"(?:^|[;{]\s*)(?:[A-Za-z_][\w.<>]*(?:\[\])?)\s+([A-Za-z_]\w*)\s*=[^=]", body, re.M)
    assert {"result", "q"} <= set(locals_), locals_
    for name in locals_:
        first = re.search(r"\b" + name + r"\b", body).start()
        decl = re.search(r"[\w.<>\]]\s+" + name + r"\s*=[^=]", body).start()
        assert first > decl, (name, "is used before the line that declares it")
    assert re.search(r"^\s*RtParams\s+p\s*;", backend, re.M) and "p" not in locals_        # the field Gather reads
    assert re.search(r"samples\s*=\s*p\.numRaysPerPixel", body)


def test_python_default_samples_follow_the_params(rtx):
    """samples=None with a mode (gather(points, mode=GATHER_SH9)) is the numRaysPerPixel of the params set last; nothing at all is NULL"""
    g = rtx._cabi._gather_params
    assert g(None, 0, 0, 0) is None and g(None, 0, 0, 0, 7) is None
    q = g(None, 0, 0, rtx.GATHER_SH9, 7)
    assert (int(q["samples"]), int(q["mode"]), int(q["seed"]), int(q["firstIndex"])) == (7, 1, 0, 0)
    assert int(g(None, 5, 0, 0, 3)["samples"]) == 3 and int(g(9, 5, 0, 1, 3)["samples"]) == 9
    with pytest.raises(TypeError):
        g(None, 0, 0, rtx.GATHER_SH9)
    assert rtx._cabi._gather_shape(4, q) == (4, 9, 4) and rtx._cabi._gather_shape(4, None) == (4, 4)


def test_gather_kernels_are_built_without_scratch():
    names = set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_gather" not in k[".name"] or "ploc" in k[".name"]:        # (k_ploc_gather is the BVH builder's)
                continue
            names.add(k[".name"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (k[".name"], "scratch")
    assert len(names) == 4, sorted(names)           # cosine / SH9 x f16 / f32 nodes
