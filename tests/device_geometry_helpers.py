"""What the device-geometry tests share: device memory without torch (the HIP runtime the library has loaded, through ctypes), the
small scenes, and the snapshot of everything a context computes from a scene — frames of both kernels and both RNG modes, the ray,
closest-point and multi-hit queries, the feature planes — as bytes.  Test infrastructure only."""
import ctypes

import numpy as np

from bvh_audit import awkward_triangles
from ray_query_helpers import camera_rays, make_rays, random_rays

COUNTS = [1, 2, 5, 64, 65, 257]          # a leaf, a node, the awkward five, a treelet boundary either side, more than one block
W, H = 32, 24


class DeviceMemory:
    """hipMalloc'ed copies of host arrays; everything is freed on exit.  hipMemcpy from pageable host memory has completed when it
    returns, so a buffer's contents are ordered before any upload that follows."""

    def __init__(self):
        with open("/proc/self/maps") as maps:
            paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
        assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
        self.hip = ctypes.CDLL(paths.pop())
        self.ptrs = []

    def put(self, tris):
        """-> (device pointer, n) of a copy of the TRIANGLE array `tris`"""
        a = np.ascontiguousarray(tris)
        p = ctypes.c_void_p(0)
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(a.nbytes, 72))) == 0
        self.ptrs.append(p)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return int(p.value), len(a)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def small_scene(rtx, n, far=0.0):
    """(params, spheres, triangles, meshinfo): n awkward triangles (n >= 5: an exact duplicate, a NaN coordinate, and the last triangle in
    no chunk) and one sphere, seen by the mesh-test scene's camera at 32 x 24; `far` moves all of it, camera included, along x.  The chunk's
    box is wide enough for every deformation the tests make, so the meshinfo never has to follow."""
    params = rtx.scenes.mesh_test_scene(W, H).build_buffers()[0].copy()
    params["numRaysPerPixel"], params["maxBounceCount"] = 2, 3
    tris, infos = awkward_triangles(rtx, n)
    if n >= 5:
        infos["numTriangles"] = n - 1
    infos["boundsMin"], infos["boundsMax"] = -1.0e6, 1.0e6
    spheres = np.zeros(1, rtx.SPHERE)
    spheres["position"], spheres["radius"] = (0.5, 1.0, 1.5), 0.4
    spheres["material"]["colour"] = (0.9, 0.2, 0.2, 1)
    if far:
        shift = np.float32([far, 0, 0])
        for k in ("posA", "posB", "posC"):
            tris[k] = tris[k] + shift
        spheres["position"] = spheres["position"] + shift
        pos = np.asarray(params["worldSpaceCameraPos"], np.float32) + shift
        params["worldSpaceCameraPos"] = pos
        m = params["camLocalToWorld"].copy(); m[3], m[7], m[11] = pos; params["camLocalToWorld"] = m
    return params, spheres, tris, infos


def displaced(tris, step, amplitude=0.15):
    """the triangles after `step` steps of a smooth displacement field (corners move, normals are turned a little too)"""
    out = tris.copy()
    for k in ("posA", "posB", "posC"):
        p = np.asarray(tris[k], np.float32)
        d = np.stack([np.sin(p[:, 1] * 1.3 + step), np.cos(p[:, 0] * 0.7 + 0.5 * step), np.sin(p[:, 2] + p[:, 0] + step)], 1)
        out[k] = (p + np.float32(amplitude * step) * d.astype(np.float32)).astype(np.float32)
    for k in ("normalA", "normalB", "normalC"):
        out[k] = (np.asarray(tris[k], np.float32) + np.float32(0.01 * step)).astype(np.float32)
    return out


def query_rays(rtx, params, spheres, tris, seed=5):
    with np.errstate(invalid="ignore"):
        finite = tris[np.isfinite(np.asarray(tris["posA"])).all(1) & np.isfinite(np.asarray(tris["posB"])).all(1)]
    return np.concatenate([camera_rays(rtx, params, 16, 12), random_rays(rtx, finite, spheres, 300, seed)])


def snapshot(rtx, t, params, rays, frames=True):
    """everything `t` computes from the scene it holds, as bytes by name"""
    out = {}
    if frames:
        for kernel in (0, 1):
            for rng in (0, 1):
                p = params.copy(); p["rngMode"] = rng
                t.set_option("kernel", kernel)
                t.set_params(p)
                t.reset_accum()
                t.render(0, 2)
                out[f"frames kernel {kernel} rng {rng}"] = t.read_accum().tobytes()
        t.set_option("kernel", -1)
        t.set_params(params)
        t.reset_aov()
        t.render_aov(0, 2)
        for which in range(rtx._cabi.RT_AOV_COUNT):
            out[f"aov {which}"] = t.read_aov(which).tobytes()
    else:
        t.set_params(params)
    out["trace_rays"] = t.trace_rays(rays).tobytes()
    out["occluded"] = t.occluded(rays).tobytes()
    out["closest_points"] = t.closest_points(rays).tobytes()
    out["trace_hits"] = t.trace_hits(rays, max_hits=4, both_sides=True).tobytes()
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, f"{what}: {bad} differ"


def fresh_snapshot(rtx, scene, rays, frames=True, **options):
    """the snapshot of a new context given `scene` from host memory, built on the device"""
    params, spheres, tris, infos = scene
    with rtx.Tracer(0) as t:
        t.set_option("device_bvh", 1)
        for k, v in options.items():
            t.set_option(k, v)
        t.set_params(params)
        t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
        return snapshot(rtx, t, params, rays, frames)
