"""Closest-point queries without a GPU: the checker (tests/closest_oracle.c) is pinned independently of the kernel — against a float64
twin of the definition that takes another route to the minimum, and against hand-computed cases on power-of-two coordinates — and the
boundary is checked: sizes, exports, bindings, the four k_closest instantiations without scratch.

(1) Float64 twin, and the tolerance on dst.  eps = 2^-24.  Let L bound |eAB|, |eAC| and |ap| of a case and N2 = |cross(eAB, eAC)|^2 of
its worst triangle.  In the checker's float32: a component of eAB or ap carries one rounding, a dot of two such vectors three products
and two sums: |error of d_i| <= 6 eps L^2.  va, vb, vc are differences of two products of d's: <= 2 (2 * 6 eps L^2 * L^2 + eps L^4) +
2 eps L^4 = 28 eps L^4 each; den, their sum: <= 3 * 28 eps L^4 + 6 eps L^4 = 90 eps L^4.  A quotient u = vb / den with den = N2 (1 + ...):
|error of u| <= (28 + 90) eps L^4 / N2 + eps, the same for v and (smaller) for the edge quotients.  The point q moves by at most
(|du| + |dv|) L, and the distance from p to a point of the triangle that lies |dq| from the closest one is at most |dq| larger (it
cannot be smaller than the minimum by more than the rounding of q, e and k themselves: 8 eps (|p| + L)).  So
    tol = 2 (118 eps L^4 / N2 + eps) L + 8 eps (|p| + L)
per case, from the case's inputs alone (L and N2 are measured on the case in float64).  The cases keep it small: edges of 1 to 2, angles
of 30 to 150 degrees at A (N2 >= 0.25), points and vertices A in [-1, 1]^3 (|ap| <= 2 sqrt 3): at most 0.03, typically 1e-3.  The twin may name another primitive only where its own two best distances lie within tol of each other; the share of such
cases is printed and capped at 1 %."""
import ctypes
import os
import re

import numpy as np
import pytest

import closest_check as cc
from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_closest_points", "rt_closest_points_device", "rt_get_closest_info", "rt_multi_closest_points")
EPS = 2.0 ** -24


def scene(rtx, tris=(), spheres=(), chunks=None):
    """(spheres, triangles, meshinfo): triangles as (A, B, C) triples with the normal (0, 0, 1) at every vertex, spheres as (centre,
    radius); one chunk over all triangles unless chunks = [(first, count), ...]"""
    t = np.zeros(len(tris), rtx.TRIANGLE)
    for i, (A, B, C) in enumerate(tris):
        t["posA"][i], t["posB"][i], t["posC"][i] = A, B, C
    t["normalA"] = t["normalB"] = t["normalC"] = (0.0, 0.0, 1.0)
    s = np.zeros(len(spheres), rtx.SPHERE)
    for i, (c, r) in enumerate(spheres):
        s["position"][i], s["radius"][i] = c, r
    chunks = ([(0, len(tris))] if len(tris) else []) if chunks is None else chunks
    m = np.zeros(len(chunks), rtx.MESHINFO)
    for i, (first, count) in enumerate(chunks):
        m["firstTriangleIndex"][i], m["numTriangles"][i] = first, count
    return s, t, m


def one(rtx, sc, p, R=np.inf):
    return cc.oracle_closest(rtx, *sc, cc.points_of(rtx, [p], R))[0]


T0 = ((0, 0, 0), (4, 0, 0), (0, 4, 0))
T1 = ((4, 0, 0), (4, 4, 0), (0, 4, 0))

# (point, dst, closest point, u, v, side): every region of T0, hand-computed (the module docstring of closest_oracle.c names the formulas)
REGIONS = {
    "vertex A": ((-3, -4, 0), 5.0, (0, 0, 0), 0.0, 0.0, 0),
    "vertex B": ((7, -4, 0), 5.0, (4, 0, 0), 1.0, 0.0, 0),
    "vertex C": ((-4, 7, 0), 5.0, (0, 4, 0), 0.0, 1.0, 0),
    "edge AB": ((2, -3, 0), 3.0, (2, 0, 0), 0.5, 0.0, 0),
    "edge AC": ((-3, 2, 0), 3.0, (0, 2, 0), 0.0, 0.5, 0),
    "edge BC": ((4, 4, 1), 3.0, (2, 2, 0), 0.5, 0.5, 1),
    "interior, front": ((1, 1, 2), 2.0, (1, 1, 0), 0.25, 0.25, 1),
    "interior, back": ((1, 1, -2), 2.0, (1, 1, 0), 0.25, 0.25, -1),
    "on vertex B": ((4, 0, 0), 0.0, (4, 0, 0), 1.0, 0.0, 0),
    "on edge AB": ((2, 0, 0), 0.0, (2, 0, 0), 0.5, 0.0, 0),
    "in the interior": ((1, 1, 0), 0.0, (1, 1, 0), 0.25, 0.25, 0),
}


@pytest.mark.parametrize("name", list(REGIONS))
def test_the_seven_regions_and_zero_distances(rtx, name):
    p, dst, q, u, v, side = REGIONS[name]
    r = one(rtx, scene(rtx, [T0]), p)
    assert r["kind"] == 2 and r["primitive"] == 0 and r["chunk"] == 0 and r["mesh"] == -1
    assert r["dst"] == np.float32(dst) and tuple(r["point"]) == q and r["u"] == u and r["v"] == v and r["side"] == side, r
    assert tuple(r["normal"]) == (0, 0, 1) and (r["_reserved"] == 0).all()


def test_spheres_from_outside_and_inside(rtx):
    sc = scene(rtx, spheres=[((0, 0, 0), 2.0)])
    out_, in_ = one(rtx, sc, (0, 0, 4)), one(rtx, sc, (0, 0, 1))
    for r, dst, side in ((out_, 2.0, 1), (in_, 1.0, -1)):
        assert r["kind"] == 1 and r["primitive"] == 0 and r["chunk"] == -1 and r["mesh"] == -1 and r["u"] == 0 and r["v"] == 0
        assert r["dst"] == dst and tuple(r["point"]) == (0, 0, 2) and tuple(r["normal"]) == (0, 0, 1) and r["side"] == side, r
    # on the centre: whatever the arithmetic gives (r / 0 = inf, 0 * inf = NaN), and no fault
    c = one(rtx, sc, (0, 0, 0))
    assert c["kind"] == 1 and c["dst"] == 2.0 and np.isnan(c["point"]).all() and c["side"] == -1


def test_degenerate_triangles(rtx):
    r = one(rtx, scene(rtx, [((1, 1, 1), (1, 1, 1), (1, 1, 1))]), (1, 1, 3))
    assert r["kind"] == 2 and r["dst"] == 2.0 and tuple(r["point"]) == (1, 1, 1) and r["u"] == 0 and r["v"] == 0 and r["side"] == 0
    r = one(rtx, scene(rtx, [((0, 0, 0), (2, 0, 0), (4, 0, 0))]), (1, 2, 0))
    assert r["kind"] == 2 and r["dst"] == 2.0 and tuple(r["point"]) == (1, 0, 0) and r["u"] == 0.5 and r["v"] == 0 and r["side"] == 0
    # beyond the far end of the collinear triangle: vertex C
    r = one(rtx, scene(rtx, [((0, 0, 0), (2, 0, 0), (4, 0, 0))]), (8, 3, 0))
    assert r["dst"] == 5.0 and tuple(r["point"]) == (4, 0, 0) and r["v"] == 1.0


def test_the_radius_is_strict(rtx):
    sc = scene(rtx, [T0], [((1, 1, -6), 2.0)])          # triangle at 2 (key 4), sphere at 6 (key 36) from (1, 1, 2)
    p = (1, 1, 2)
    assert one(rtx, sc, p, 2.0)["kind"] == 0 and one(rtx, sc, p, np.nextafter(np.float32(2), np.float32(3)))["kind"] == 2
    miss = one(rtx, sc, p, 2.0)
    assert np.isposinf(miss["dst"]) and (miss["point"] == 0).all() and (miss["normal"] == 0).all() and miss["primitive"] == -1 \
        and miss["chunk"] == -1 and miss["mesh"] == -1 and miss["u"] == 0 and miss["v"] == 0 and miss["side"] == 0
    assert one(rtx, sc, p, np.inf)["kind"] == 2 and one(rtx, sc, p, 1e30)["kind"] == 2      # (R * R = +inf: unbounded)


def test_ties_lower_index_and_sphere_first(rtx):
    for tris in ([T0, T1], [T1, T0]):
        r = one(rtx, scene(rtx, tris), (2, 2, 1))
        assert r["kind"] == 2 and r["primitive"] == 0 and r["dst"] == 1.0 and tuple(r["point"]) == (2, 2, 0), r
    # the same through two chunks listed out of order: the uploaded index decides, not the chunk order
    r = one(rtx, scene(rtx, [T0, T1], chunks=[(1, 1), (0, 1)]), (2, 2, 1))
    assert r["primitive"] == 0 and r["chunk"] == 1
    # a sphere and a triangle at key 4: the sphere wins, wherever it sits in its buffer
    r = one(rtx, scene(rtx, [T0], [((9, 9, 9), 1.0), ((1, 1, 6), 2.0)]), (1, 1, 2))
    assert r["kind"] == 1 and r["primitive"] == 1 and r["dst"] == 2.0
    # two spheres at the same key: the lower index
    r = one(rtx, scene(rtx, spheres=[((0, 0, 4), 2.0), ((0, 0, -4), 2.0)]), (0, 0, 0))
    assert r["kind"] == 1 and r["primitive"] == 0


def test_points_and_radii_that_are_not_searched(rtx):
    sc = scene(rtx, [T0], [((0, 0, 8), 1.0)])
    for p, R in (((np.nan, 1, 1), np.inf), ((1, np.inf, 1), np.inf), ((1, 1, 2), 0.0), ((1, 1, 2), -1.0), ((1, 1, 2), np.nan)):
        r = one(rtx, sc, p, R)
        assert r["kind"] == 0 and np.isposinf(r["dst"]) and r["primitive"] == -1 and r["side"] == 0, (p, R, r)
    # a triangle no chunk addresses is no candidate
    r = one(rtx, scene(rtx, [T0, T1], chunks=[(1, 1)]), (1, 1, 2))
    assert r["primitive"] == 1
    empty = cc.oracle_closest(rtx, *scene(rtx), cc.points_of(rtx, [(0, 0, 0)]))
    assert empty[0]["kind"] == 0


def _random_case(rng, nt=4, ns=2):
    """well-shaped triangles around the origin: edges of 1 to 2 with at least 30 degrees between them at A, so that N2 >= 0.25"""
    A, B, C = np.zeros((nt, 3)), np.zeros((nt, 3)), np.zeros((nt, 3))
    for i in range(nt):
        while True:
            a = rng.uniform(-1, 1, 3)
            d1, d2 = rng.standard_normal(3), rng.standard_normal(3)
            d1, d2 = d1 / np.linalg.norm(d1), d2 / np.linalg.norm(d2)
            if abs(np.dot(d1, d2)) <= np.cos(np.pi / 6):
                break
        A[i], B[i], C[i] = a, a + d1 * rng.uniform(1, 2), a + d2 * rng.uniform(1, 2)
    c = rng.uniform(-1, 1, (ns, 3))
    r = rng.uniform(0.25, 1.0, ns)
    p = rng.uniform(-1, 1, 3)
    return A.astype(np.float32), B.astype(np.float32), C.astype(np.float32), c.astype(np.float32), r.astype(np.float32), p.astype(np.float32)


def test_checker_against_the_float64_twin(rtx):
    rng = np.random.default_rng(20260)
    cases, excused, worst = 2000, 0, 0.0
    for _ in range(cases):
        A, B, C, c, r, p = _random_case(rng)
        sc = scene(rtx, list(zip(A, B, C)), list(zip(c, r)))
        got = one(rtx, sc, p)
        k, kind, prim, dst = cc.twin64(p, np.inf, c, r, A, B, C)
        A64, B64, C64, p64 = A.astype(np.float64), B.astype(np.float64), C.astype(np.float64), p.astype(np.float64)
        L = max(np.linalg.norm(B64 - A64, axis=1).max(), np.linalg.norm(C64 - A64, axis=1).max(), np.linalg.norm(p64 - A64, axis=1).max())
        N2 = (np.cross(B64 - A64, C64 - A64) ** 2).sum(1).min()
        assert L <= 2 + 2 * np.sqrt(3) + 1e-6 and N2 >= 0.25 * (1 - 1e-5)      # (what the docstring's figures assume; float32 inputs)
        tol = 2 * (118 * EPS * L ** 4 / N2 + EPS) * L + 8 * EPS * (np.linalg.norm(p64) + L)
        worst = max(worst, abs(float(got["dst"]) - dst))
        assert abs(float(got["dst"]) - dst) <= tol, (got, dst, tol)
        if (int(got["kind"]), int(got["primitive"])) != (int(kind[0]), int(prim[0])):
            assert len(k) > 1 and np.sqrt(k[1]) - np.sqrt(k[0]) <= tol, (got, k[:2], kind[:2], prim[:2])
            excused += 1
    print(f"twin: {cases} cases, largest |dst - twin| {worst:.3e}, near ties excused {excused} ({100.0 * excused / cases:.2f} %)")
    assert excused <= cases // 100


def test_checker_against_the_twin_with_a_radius(rtx):
    """the radius drops the same candidates in both: a miss in one is a miss in the other unless the winner's distance is within the
    tolerance of R"""
    rng = np.random.default_rng(7)
    misses = 0
    for _ in range(400):
        A, B, C, c, r, p = _random_case(rng)
        R = np.float32(rng.uniform(0.05, 0.6))
        got = one(rtx, scene(rtx, list(zip(A, B, C)), list(zip(c, r))), p, R)
        k, kind, prim, dst = cc.twin64(p, R, c, r, A, B, C)
        full = cc.twin64(p, np.inf, c, r, A, B, C)[3]
        if (got["kind"] == 0) != (len(k) == 0):
            assert abs(full - float(R)) <= 1e-3, (got, full, R)
        misses += int(got["kind"] == 0)
        assert got["kind"] == 0 or float(got["dst"]) < float(R)
    assert 40 < misses < 360


# ---- boundary ---------------------------------------------------------------------------------------------------------------------------
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
        assert hasattr(cls, "closest_points")
    assert hasattr(rtx.Tracer, "closest_points_device") and hasattr(rtx.Tracer, "closest_info")
    assert hasattr(rtx.RayTracingManager, "ClosestPoints")
    assert hasattr(rtx.host_cpp_binding.CppScene, "closest_points")
    text = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert '"closest_slice"' in text and '"closest_count"' in text
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    assert lib.rt_sizeof(b"rt_closest") == 64 == rtx.CLOSEST.itemsize
    assert lib.rt_sizeof(b"rt_closest_info") == 40 == rtx.CLOSEST_INFO.itemsize
    header = _header()
    for name, dt in (("rt_closest", rtx.CLOSEST), ("rt_closest_info", rtx.CLOSEST_INFO)):
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)
    assert rtx.CLOSEST.names == ("dst", "point", "normal", "kind", "primitive", "chunk", "mesh", "u", "v", "side", "_reserved")
    assert rtx.CLOSEST_INFO.names == ("calls", "_reserved", "lastKernelMs", "totalKernelMs", "lastNodeSteps", "lastPrimTests")
    # the C compiler's layout of the header's text, through ctypes

    class CClosest(ctypes.Structure):
        _fields_ = [("dst", ctypes.c_float), ("point", ctypes.c_float * 3), ("normal", ctypes.c_float * 3), ("kind", ctypes.c_int32),
                    ("primitive", ctypes.c_int32), ("chunk", ctypes.c_int32), ("mesh", ctypes.c_int32), ("u", ctypes.c_float),
                    ("v", ctypes.c_float), ("side", ctypes.c_int32), ("_reserved", ctypes.c_int32 * 2)]

    class CInfo(ctypes.Structure):
        _fields_ = [("calls", ctypes.c_int32), ("_reserved", ctypes.c_int32), ("lastKernelMs", ctypes.c_double), ("totalKernelMs", ctypes.c_double),
                    ("lastNodeSteps", ctypes.c_uint64), ("lastPrimTests", ctypes.c_uint64)]
    for cs, dt in ((CClosest, rtx.CLOSEST), (CInfo, rtx.CLOSEST_INFO)):
        assert ctypes.sizeof(cs) == dt.itemsize
        for f, _ in cs._fields_:
            assert getattr(cs, f).offset == dt.fields[f][1], f


def test_csharp_closest_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtClosest.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtClosest": ("rt_closest", rtx.CLOSEST), "RtClosestInfo": ("rt_closest_info", rtx.CLOSEST_INFO)}
    assert set(structs) == set(pairs)
    for cs_name, (c_name, dt) in pairs.items():
        rows, size, _ = _layout(structs, cs_name)
        assert size == lib.rt_sizeof(c_name.encode()) == dt.itemsize, (cs_name, size)
        assert [r[0] for r in rows] == list(dt.names), (cs_name, rows)
        for field, off, nbytes in rows:
            assert off == dt.fields[field][1] and nbytes == dt.fields[field][0].itemsize, (cs_name, field, off, nbytes)


def test_csharp_backend_and_compiled_host_reach_the_entry_points():
    native, backend = open(os.path.join(CS, "RtNative.cs")).read(), open(os.path.join(CS, "RtBackend.cs")).read()
    sig = {"rt_closest_points": r"IntPtr ctx, \[In\] RtRay\[\] points, int n, \[Out\] RtClosest\[\] result",
           "rt_closest_points_device": r"IntPtr ctx, IntPtr points, int n, IntPtr result",
           "rt_get_closest_info": r"IntPtr ctx, out RtClosestInfo info",
           "rt_multi_closest_points": r"IntPtr multi, \[In\] RtRay\[\] points, int n, \[Out\] RtClosest\[\] result"}
    for name in EXPORTS:
        assert re.search(r"static\s+extern\s+int\s+" + name + r"\s*\(" + sig[name] + r"\)", native), name
    used = set(re.findall(r"RtNative\.(\w+)", backend))
    assert {"rt_closest_points", "rt_multi_closest_points"} <= used
    assert re.search(r"public\s+RtClosest\[\]\s+ClosestPoints\s*\(\s*RtRay\[\]\s+points", backend)
    for name in ("rt_closest", "rt_closest_info"):
        assert '"' + name + '"' in native, name                               # VerifyLayout
    host = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
    hpp = open(os.path.join(host, "rt_host.hpp")).read()                      # one declaration, for either handle kind
    assert "ClosestPoints(Target " in hpp and "Target(rt_ctx* " in hpp and "Target(rt_multi* " in hpp
    assert "rth_closest_points" in open(os.path.join(host, "rt_host_c.cpp")).read()


def test_the_compiled_host_refuses_bad_arguments_before_it_touches_a_device(rtx):
    L = rtx.host_cpp_binding.load_host_library()
    assert L.rth_closest_points(None, None, 0, None, -1, None) == -1 and b"rth_closest_points" in L.rth_last_error()


def test_closest_kernels_are_built_without_scratch():
    names = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_closest" not in k[".name"]:
                continue
            names[k[".name"]] = k[".vgpr_count"]
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
    print("k_closest VGPRs:", names)
    assert len(names) == 4, sorted(names)           # f16 / f32 nodes x plain / counting
