"""Visibility gathers without a GPU: the checker (tests/query_oracle.c: the oracle's own random_direction() and
calculate_ray_collision() per point and sample) is pinned to the gather checker's directions, to the ray-query checker, to the tree restated
in numpy and to exact and statistical cases, and the ABI is declared, exported and bound.

One bound is not the one the feature request words.  It asks that coefficient 0 of the SH9 of an empty scene be "within 5 standard errors
of 4 pi Y0", the standard error computed from the basis function's variance over the sphere.  Y0 is a constant: its variance, and with it
the bound, is zero, while the float32 tree that adds the same value N = 4096 times rounds (the gather tests record -15 to -23 ulp for such
sums).  The test keeps the statistical term as asked (it computes it, and it is 0 to quadrature error) and adds the rounding of the
number format, derived and not measured: N / S - 1 = 255 additions in a sub-stream, log2 S = 4 in the tree, one division and one
multiplication, each at most 2^-24 of a value no larger than the result: 261 * 2^-24 = 1.56e-5 relative."""
import os
import re

import numpy as np
import pytest

import query_check as gc
import query_check as vc
from query_check import oracle_hits
from ray_query_helpers import camera_rays, make_rays, shim  # noqa: F401  (shim: a fixture)
from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_gather_cpu import inward_box, triangle_scene
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata
from test_radiance_cpu import light_scene

EXPORTS = ("rt_visibility", "rt_visibility_device", "rt_get_visibility_info", "rt_multi_visibility")
COUNTS = [1, 3, 4, 5, 16, 17, 21, 64]
f32 = np.float32


def point(rtx, origin, normal, t=np.inf):
    return make_rays(rtx, [origin], [normal], t)


def empty(rtx):
    return np.zeros(0, rtx.SPHERE), np.zeros(0, rtx.TRIANGLE), np.zeros(0, rtx.MESHINFO)


# ---- 1. directions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, gather_mode", [(vc.COSINE, gc.COSINE), (vc.DISTANCE, gc.COSINE), (vc.SH9, gc.SH9)])
def test_directions_are_the_gather_queries_directions(rtx, mode, gather_mode):
    normals = ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.6, 0.0, -0.8), (3.0, -2.0, 0.5), (np.nan, 5.0, -2.0))
    for normal in normals:
        for sample, seed, index in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (9, 678, 12345), (65535, 0xFFFFFFFF, 0xFFFFFFFF)):
            vc.assert_same_bits(vc.direction(normal, sample, seed, index, mode), gc.direction(normal, sample, seed, index, gather_mode),
                                f"mode {mode} normal {normal} ({sample}, {seed}, {index})")
    assert (vc.direction(normals[1], 0, 0, 0, vc.COSINE) != vc.direction(normals[1], 0, 0, 0, vc.SH9)).any()


# ---- 2. a sample is the ray-query checker's answer along the drawn direction ---------------------------------------------------------
@pytest.fixture(scope="module")
def batch(rtx, shim):  # noqa: F811
    params, spheres, tris, infos = light_scene(rtx)
    hits = oracle_hits(rtx, shim, spheres, tris, infos, 0, camera_rays(rtx, params)[7::211])
    pts = vc.surface_points(rtx, hits)
    assert 8 <= len(pts) <= 16 and (pts["direction"] != 0).any(1).sum() >= 4
    pts["tMax"][1::3] = f32(2.5)                                                     # a reach that rejects some hits
    return spheres, tris, infos, pts


@pytest.mark.parametrize("intersect", [0, 1])
def test_samples_are_the_ray_query_checkers_answers(rtx, shim, batch, intersect):  # noqa: F811
    spheres, tris, infos, pts = batch
    N, seed, first = 5, 9, 1000
    seen = set()
    for mode in vc.MODES:
        rays = vc.sample_rays(rtx, pts, N, seed, first, mode)
        hits = oracle_hits(rtx, shim, spheres, tris, infos, intersect, rays).reshape(len(pts), N)
        free = oracle_hits(rtx, shim, spheres, tris, infos, intersect, make_rays(rtx, rays["origin"], rays["direction"])).reshape(len(pts), N)
        for i in range(len(pts)):
            for s in range(N):
                got = vc.oracle_visibility_sample(rtx, spheres, tris, infos, pts[i:i + 1], s, seed, first + i, mode, intersect)
                occ = hits["kind"][i, s] != 0
                seen.add((mode, bool(occ)))
                seen.add(("bounded away", bool(free["kind"][i, s] != 0 and not occ)))
                if mode == vc.DISTANCE:
                    r = hits["dst"][i, s] if occ else pts["tMax"][i]
                    vc.assert_same_bits(got, np.array([r, f32(r) * f32(r), 1.0 if occ else 0.0], f32), f"point {i} sample {s}")
                    continue
                assert got[-1] == (0.0 if occ else 1.0), (mode, i, s)
                d = rays["direction"].reshape(len(pts), N, 3)[i, s]
                want = gc.sh_basis(d) if mode == vc.SH9 else d
                vc.assert_same_bits(got[:-1], want if not occ else np.zeros_like(want), f"mode {mode} point {i} sample {s}")
    assert {(m, o) for m in vc.MODES for o in (True, False)} <= seen and ("bounded away", True) in seen


def test_the_search_tree_does_not_change_the_checker(rtx, batch):
    spheres, tris, infos, pts = batch
    for mode in vc.MODES:
        for intersect in (0, 1):
            a = vc.oracle_visibility(rtx, spheres, tris, infos, pts, 5, 1, 2, mode, intersect, accel=True)
            b = vc.oracle_visibility(rtx, spheres, tris, infos, pts, 5, 1, 2, mode, intersect, accel=False)
            vc.assert_same_bits(a, b, f"tree against loop, mode {mode} intersect {intersect}")


# ---- 3. the tree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_the_tree_is_the_written_rule(rtx, batch, n):
    spheres, tris, infos, pts = batch
    seed, first = 4, 0xFFFFFFFC                                                      # (the index wraps inside the batch)
    for mode in vc.MODES:
        got = vc.oracle_visibility(rtx, spheres, tris, infos, pts, n, seed, first, mode)
        varied = False
        for i in range(len(pts)):
            ch = np.stack([vc.oracle_visibility_sample(rtx, spheres, tris, infos, pts[i:i + 1], s, seed, first + i, mode) for s in range(n)])
            varied = varied or len(np.unique(ch, axis=0)) > 1
            vc.assert_same_bits(got[i], vc.finish(vc.tree_sum(ch), mode), f"N = {n}, mode {mode}, point {i}")
            count = ch[:, -1].astype(np.float64).sum()                               # the 0 / 1 channel: count / N whatever the tree
            assert got[i, {vc.COSINE: 3, vc.SH9: 9, vc.DISTANCE: 2}[mode]] == f32(count) / f32(n)
        assert varied or n == 1


def test_the_checker_is_split_invariant_under_first_index(rtx, batch):
    spheres, tris, infos, pts = batch
    first = 0xFFFFFFFA
    for mode in vc.MODES:
        whole = vc.oracle_visibility(rtx, spheres, tris, infos, pts, 5, 2, first, mode)
        for cut in (1, 6, len(pts) - 1):
            a = vc.oracle_visibility(rtx, spheres, tris, infos, pts[:cut], 5, 2, first, mode)
            b = vc.oracle_visibility(rtx, spheres, tris, infos, pts[cut:], 5, 2, first + cut, mode)
            vc.assert_same_bits(np.concatenate([a, b]), whole, f"cut at {cut}")
        assert (vc.oracle_visibility(rtx, spheres, tris, infos, pts, 5, 2, 1, mode) != whole).any()
        assert (vc.oracle_visibility(rtx, spheres, tris, infos, pts, 5, 3, first, mode) != whole).any()      # the seed


# ---- 4. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64])
def test_an_empty_scene_is_open(rtx, n):
    s, t, m = empty(rtx)
    pt = point(rtx, (0.3, -0.2, 0.1), (0.0, 0.0, 1.0), 3.0)
    cos = vc.oracle_visibility(rtx, s, t, m, pt, n, seed=5, mode=vc.COSINE)[0]
    assert cos[3] == 1.0 and cos[2] > 0.0                                            # open, bent towards the normal
    assert vc.oracle_visibility(rtx, s, t, m, pt, n, seed=5, mode=vc.SH9)[0, 9:].tolist() == [1.0, 0.0, 0.0]
    assert vc.oracle_visibility(rtx, s, t, m, pt, n, seed=5, mode=vc.DISTANCE).tolist() == [[3.0, 9.0, 0.0, 1.0]]
    pt["tMax"] = np.inf
    assert vc.oracle_visibility(rtx, s, t, m, pt, n, seed=5, mode=vc.DISTANCE).tolist() == [[np.inf, np.inf, 0.0, 1.0]]


@pytest.fixture(scope="module")
def box(rtx):
    """a closed axis-aligned box of half-size 1 about the origin, twelve triangles that face inwards (a ray from inside a sphere never
    hits it: RaySphere keeps the near root only)"""
    _, _, tris, infos = inward_box(rtx, 1.0, (0.0, 0.0, 0.0), 0.0)
    return np.zeros(0, rtx.SPHERE), tris, infos


@pytest.mark.parametrize("intersect", [0, 1])
@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.0, 0.0, 0.0)])
def test_the_centre_of_a_closed_box(rtx, box, normal, intersect):
    N = 64
    kw = dict(samples=N, seed=3, intersect=intersect)
    centre = (0.0, 0.0, 0.0)
    # unbounded: every direction is closed
    pt = point(rtx, centre, normal)
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.COSINE, **kw).tolist() == [[0.0, 0.0, 0.0, 0.0]]
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.SH9, **kw).tolist() == [[0.0] * 12]
    dist = vc.oracle_visibility(rtx, *box, pt, mode=vc.DISTANCE, **kw)[0]
    assert dist[2] == 1.0 and dist[3] == 1.0 and 1.0 <= dist[0] <= np.sqrt(3.0) and 1.0 <= dist[1] <= 3.0
    # a reach of 0.5 ends before the nearest wall: every direction is open, every r is the reach
    pt = point(rtx, centre, normal, 0.5)
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.COSINE, **kw)[0, 3] == 1.0
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.SH9, **kw)[0, 9] == 1.0
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.DISTANCE, **kw).tolist() == [[0.5, 0.25, 0.0, 1.0]]
    # a reach of 2 is beyond the farthest corner (sqrt 3)
    pt = point(rtx, centre, normal, 2.0)
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.COSINE, **kw).tolist() == [[0.0, 0.0, 0.0, 0.0]]
    assert vc.oracle_visibility(rtx, *box, pt, mode=vc.DISTANCE, **kw)[0, 2] == 1.0


@pytest.mark.parametrize("mode", vc.MODES)
def test_points_with_no_positive_reach_are_not_traced(rtx, box, mode):
    t = np.array([0.0, -0.0, -1.0, np.nan, -np.inf, 1.0e3], f32)
    pts = make_rays(rtx, [(0.0, 0.0, 0.0)] * 6, [(0.0, 1.0, 0.0)] * 6, t)
    got = vc.oracle_visibility(rtx, *box, pts, 16, mode=mode)
    assert (got[:5].view(np.uint32) == 0).all()
    assert (got[5] != 0).any() or mode != vc.DISTANCE
    assert mode != vc.DISTANCE or got[5, 3] == 1.0


# ---- 5. statistical cases -----------------------------------------------------------------------------------------------------------
def square_form_factor(half, height):
    """the form factor from a differential element to a parallel square centred above it, in float64: four corner rectangles
    (X = Y = half / height), F_corner = (1 / 2 pi) (X / sqrt(1 + X^2) atan(Y / sqrt(1 + X^2)) + Y / sqrt(1 + Y^2) atan(X / sqrt(1 + Y^2)))"""
    X = Y = np.float64(half) / np.float64(height)
    a, b = np.sqrt(1 + X * X), np.sqrt(1 + Y * Y)
    return 4.0 * (X / a * np.arctan(Y / a) + Y / b * np.arctan(X / b)) / (2.0 * np.pi)


def test_a_square_overhead_hides_its_form_factor(rtx):
    N = 4096
    square = [[(-1, -1, 1), (1, 1, 1), (1, -1, 1)], [(-1, -1, 1), (-1, 1, 1), (1, 1, 1)]]
    _, _, tris, infos = triangle_scene(rtx, square, (0.0, 0.0, 0.0), 0.0, environment=False)
    assert (tris["normalA"] == (0, 0, -1)).all()                                      # it faces down: rays going up hit it
    F = square_form_factor(1.0, 1.0)
    assert abs(F - 0.554) < 1e-3
    p = 1.0 - F
    bound = 5.0 * np.sqrt(p * (1.0 - p) / N)
    up = point(rtx, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    for intersect in (0, 1):
        got = vc.oracle_visibility(rtx, np.zeros(0, rtx.SPHERE), tris, infos, up, N, seed=1, mode=vc.COSINE, intersect=intersect)[0]
        print(f"visibility {got[3]:.6f}, 1 - F = {p:.6f}, bound {bound:.6f}")
        assert abs(float(got[3]) - p) <= bound, (got, p, bound)
        assert got[0] != 0 and got[1] != 0 and 0 < got[2] < got[3]                  # the opening is a ring near the horizon


def basis_float64(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.28209479), 0.48860251 * y, 0.48860251 * z, 0.48860251 * x, 1.09254843 * x * y, 1.09254843 * y * z,
                     0.31539157 * (3.0 * z * z - 1.0), 1.09254843 * x * z, 0.54627421 * (x * x - y * y)], -1)


def test_the_sh9_of_an_empty_scene_is_the_constant_function(rtx):
    N = 4096
    s, t, m = empty(rtx)
    got = vc.oracle_visibility(rtx, s, t, m, point(rtx, (1.0, 2.0, 3.0), (0.0, 1.0, 0.0)), N, seed=7, mode=vc.SH9)[0]
    assert got[9] == 1.0 and got[10] == 0.0 and got[11] == 0.0
    # mean and variance of every basis function over the sphere, in float64: Gauss-Legendre in cos(theta), uniform in phi
    mu, w = np.polynomial.legendre.leggauss(32)
    phi = (np.arange(64) + 0.5) * (2.0 * np.pi / 64)
    st = np.sqrt(1.0 - mu * mu)
    d = np.stack([st[:, None] * np.cos(phi)[None, :], st[:, None] * np.sin(phi)[None, :], np.broadcast_to(mu[:, None], (32, 64))], -1)
    Y = basis_float64(d)
    weight = (w[:, None] / 2.0) * (1.0 / 64)                                          # the uniform pdf's measure: sums to 1
    mean = (Y * weight[..., None]).sum((0, 1))
    var = ((Y - mean) ** 2 * weight[..., None]).sum((0, 1))
    assert np.allclose(mean[1:], 0.0, atol=1e-9) and np.allclose(var[1:], 1.0 / (4.0 * np.pi), rtol=1e-6) and var[0] < 1e-20
    se = 4.0 * np.pi * np.sqrt(var / N)                                               # of c_k = 4 pi * the mean of N draws of Y_k
    want = 4.0 * np.pi * mean
    rounding = np.zeros(9)
    rounding[0] = 261.0 * 2.0 ** -24 * want[0]                                        # the float32 tree over a constant: the module docstring
    print("c_k", got[:9], "5 se", 5 * se)
    assert (np.abs(got[:9].astype(np.float64) - want) <= 5.0 * se + rounding).all(), (got[:9], want, se)
    assert (got[1:9] != 0).all()


# ---- 6. boundary ------------------------------------------------------------------------------------------------------------------
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
        assert hasattr(cls, "visibility")
    assert hasattr(rtx.Tracer, "visibility_device") and hasattr(rtx.Tracer, "visibility_info")
    assert hasattr(rtx.RayTracingManager, "Visibility")
    assert hasattr(rtx.host_cpp_binding.CppScene, "visibility")
    assert re.search(r"RT_VIS_COSINE\s*=\s*0\s*,\s*RT_VIS_SH9\s*=\s*1\s*,\s*RT_VIS_DISTANCE\s*=\s*2", header)
    assert re.search(r"#define\s+RT_VISIBILITY_DEFAULT_SAMPLES\s+64\b", header)
    assert (rtx.VIS_COSINE, rtx.VIS_SH9, rtx.VIS_DISTANCE) == (0, 1, 2) and rtx._cabi.VISIBILITY_DEFAULT_SAMPLES == 64
    assert '"visibility_slice"' in open(os.path.join(ROOT, "include", "rt.h")).read()
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    assert lib.rt_sizeof(b"rt_visibility_params") == 32 == rtx.VISIBILITY_PARAMS.itemsize
    assert lib.rt_sizeof(b"rt_visibility_info") == 32 == rtx.VISIBILITY_INFO.itemsize
    header = _header()
    for name, dt in (("rt_visibility_params", rtx.VISIBILITY_PARAMS), ("rt_visibility_info", rtx.VISIBILITY_INFO)):
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)
    assert rtx.VISIBILITY_PARAMS.names == ("samples", "seed", "firstIndex", "mode", "_reserved")
    assert rtx.VISIBILITY_INFO.names == ("samples", "lastSampleLanes", "calls", "mode", "lastKernelMs", "totalKernelMs")


def test_csharp_visibility_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtVisibility.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtVisibilityParams": ("rt_visibility_params", rtx.VISIBILITY_PARAMS), "RtVisibilityInfo": ("rt_visibility_info", rtx.VISIBILITY_INFO)}
    assert set(structs) == set(pairs)
    for cs_name, (c_name, dt) in pairs.items():
        rows, size, _ = _layout(structs, cs_name)
        assert size == lib.rt_sizeof(c_name.encode()) == dt.itemsize, (cs_name, size)
        assert [r[0] for r in rows] == list(dt.names), (cs_name, rows)
        for field, off, nbytes in rows:
            assert off == dt.fields[field][1] and nbytes == dt.fields[field][0].itemsize, (cs_name, field, off, nbytes)


def test_csharp_backend_and_compiled_host_reach_the_entry_points():
    native, backend = open(os.path.join(CS, "RtNative.cs")).read(), open(os.path.join(CS, "RtBackend.cs")).read()
    sig = {"rt_visibility": r"IntPtr ctx, \[In\] RtRay\[\] points, int n, \[In\] RtVisibilityParams\[\] p, \[Out\] float\[\] result",
           "rt_visibility_device": r"IntPtr ctx, IntPtr points, int n, \[In\] RtVisibilityParams\[\] p, IntPtr result",
           "rt_get_visibility_info": r"IntPtr ctx, out RtVisibilityInfo info",
           "rt_multi_visibility": r"IntPtr multi, \[In\] RtRay\[\] points, int n, \[In\] RtVisibilityParams\[\] p, \[Out\] float\[\] result"}
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(" + sig[name] + r"\)", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    assert {"rt_visibility", "rt_multi_visibility"} <= used
    assert re.search(r"public\s+float\[\]\s+Visibility\s*\(\s*RtRay\[\]\s+points", backend)
    for name in ("rt_visibility_params", "rt_visibility_info"):
        assert '"' + name + '"' in native, name                               # VerifyLayout
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "Visibility(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    assert "rth_visibility" in open(os.path.join(host, "rt_host_c.cpp")).read()


def test_the_hosts_marshal_the_same_bytes(rtx):
    """The Python binding and the compiled host's Python binding build rt_visibility_params with one function, and its bytes are the C
    struct's: four words in the header's order, then four zero words; nothing at all is NULL (the library's defaults)"""
    import ctypes

    class CParams(ctypes.Structure):                                            # include/rt.h rt_visibility_params
        _fields_ = [("samples", ctypes.c_int32), ("seed", ctypes.c_uint32), ("firstIndex", ctypes.c_uint32), ("mode", ctypes.c_int32),
                    ("_reserved", ctypes.c_int32 * 4)]
    g = rtx._cabi._visibility_params
    assert rtx.host_cpp_binding._visibility_params is g and rtx.host_cpp_binding._visibility_shape is rtx._cabi._visibility_shape
    assert g(None, 0, 0, 0) is None
    q = g(21, 0xFFFFFFFF, 0xFFFFFF00, rtx.VIS_DISTANCE)
    c = CParams(21, 0xFFFFFFFF, 0xFFFFFF00, 2)
    assert q.tobytes() == bytes(c) and ctypes.sizeof(CParams) == rtx.load_library().rt_sizeof(b"rt_visibility_params")
    assert int(g(None, 0, 0, rtx.VIS_SH9)["samples"]) == 64 and int(g(None, 5, 0, 0)["samples"]) == 64
    assert rtx._cabi._visibility_shape(4, q) == (4, 4) and rtx._cabi._visibility_shape(4, None) == (4, 4)
    assert rtx._cabi._visibility_shape(4, g(3, 0, 0, rtx.VIS_SH9)) == (4, 12)
    # the compiled host refuses bad arguments before it touches a device, through the same export
    L = rtx.host_cpp_binding.load_host_library()
    assert L.rth_visibility(None, None, 0, None, -1, None, None) == -1 and b"rth_visibility" in L.rth_last_error()


def test_visibility_kernels_are_built_without_scratch():
    names = set()
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_visibility" not in k[".name"]:
                continue
            names.add(k[".name"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, (k[".name"], "scratch")
    assert len(names) == 6, sorted(names)           # cosine / SH9 / distance x f16 / f32 nodes
