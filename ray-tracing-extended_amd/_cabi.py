"""ctypes binding of include/rt.h (the C-ABI of the HIP path tracer) plus the buffer layouts as numpy dtypes.

The layouts are the reference's own GPU-buffer structs (Assets/Scripts/Data Types/RayTracingMaterial.cs:13-19,
Sphere.cs:5-7, Triangle.cs:8-14, MeshInfo.cs:5-9; strides asserted below: 64 / 80 / 72 / 96 bytes).

There is no CPU fallback: if the HIP library has not been built, or no GPU is present, this module raises.

A new entry point of rt.h takes one line in the signature table (_declare below) and one method on the class it belongs to.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTX_LIB") or os.path.join(_HERE, "librt_mi355x.so")   # RTX_LIB: A/B builds of the same ABI

# ---- buffer layouts ------------------------------------------------------------------------------------------
MATERIAL = np.dtype([
    ("colour", "<f4", 4), ("emissionColour", "<f4", 4), ("specularColour", "<f4", 4),
    ("emissionStrength", "<f4"), ("smoothness", "<f4"), ("specularProbability", "<f4"), ("flag", "<i4"),
])
SPHERE = np.dtype([("position", "<f4", 3), ("radius", "<f4"), ("material", MATERIAL)])
TRIANGLE = np.dtype([("posA", "<f4", 3), ("posB", "<f4", 3), ("posC", "<f4", 3),
                     ("normalA", "<f4", 3), ("normalB", "<f4", 3), ("normalC", "<f4", 3)])
MESHINFO = np.dtype([("firstTriangleIndex", "<u4"), ("numTriangles", "<u4"), ("material", MATERIAL),
                     ("boundsMin", "<f4", 3), ("boundsMax", "<f4", 3)])
PARAMS = np.dtype([
    ("width", "<i4"), ("height", "<i4"), ("maxBounceCount", "<i4"), ("numRaysPerPixel", "<i4"),
    ("defocusStrength", "<f4"), ("divergeStrength", "<f4"), ("viewParams", "<f4", 3),
    ("camLocalToWorld", "<f4", 16), ("worldSpaceCameraPos", "<f4", 3), ("worldSpaceLightPos0", "<f4", 3),
    ("environmentEnabled", "<i4"), ("groundColour", "<f4", 4), ("skyColourHorizon", "<f4", 4),
    ("skyColourZenith", "<f4", 4), ("sunFocus", "<f4"), ("sunIntensity", "<f4"),
    ("rngMode", "<i4"), ("intersectMode", "<i4"),
])
STATS = np.dtype([
    ("numRenderedFrames", "<i4"), ("numMeshChunks", "<i4"), ("numTriangles", "<i4"), ("numSpheres", "<i4"),
    ("numBvhNodes", "<i4"), ("bvhMaxStack", "<i4"),
    ("rays", "<u8"), ("sphereTests", "<u8"), ("nodeVisits", "<u8"), ("triTests", "<u8"), ("hits", "<u8"),
    ("phaseLanes", "<u8", 5), ("phaseExecs", "<u8", 5),
    ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8"), ("lastGeometryMs", "<f8"), ("lastDisplayMs", "<f8"), ("lastFramesPerLaunch", "<i4"), ("autoKernel", "<i4"),
    ("lastKernel", "<i4"), ("lastFramesInterleaved", "<i4"),
    ("lastBvhBuildMs", "<f8"), ("refitAreaRatio", "<f4"), ("bvhInternalArea", "<f4"), ("bvhBuiltOnDevice", "<i4"), ("bvhBuilds", "<i4"),
    ("bvhRebuilds", "<i4"), ("bvhRepads", "<i4"), ("lastSampleLanes", "<i4"), ("queuedLaunches", "<i4"), ("regionExecs", "<u8", 32),
    ("primaryLists", "<u4", 4), ("primaryListBuilds", "<i4"), ("_reserved", "<i4"), ("lastPrimaryListsMs", "<f8"),
])
MESH_TRANSFORM = np.dtype([("position", "<f4", 3), ("rotation", "<f4", 4), ("lossyScale", "<f4", 3)])
MULTI_INFO = np.dtype([("numContexts", "<i4"), ("bvhBuilds", "<i4"), ("lastSetupMs", "<f8"), ("lastGatherMs", "<f8"),
                       ("device", "<i4", 16), ("peerAccess", "<i4", 16)])
LOCAL_CHUNK = np.dtype([("firstTriangleIndex", "<u4"), ("numTriangles", "<u4"), ("meshIndex", "<u4"), ("_reserved", "<u4"),
                        ("material", MATERIAL)])
# ray queries (rt_trace_rays / rt_occluded): a caller's ray and what it hits
RAY = np.dtype([("origin", "<f4", 3), ("tMax", "<f4"), ("direction", "<f4", 3), ("_reserved", "<i4")])
HIT = np.dtype([("dst", "<f4"), ("hitPoint", "<f4", 3), ("normal", "<f4", 3), ("kind", "<i4"), ("primitive", "<i4"), ("chunk", "<i4"),
                ("mesh", "<i4"), ("u", "<f4"), ("v", "<f4"), ("_reserved", "<i4", 3)])
RT_HIT_NONE, RT_HIT_SPHERE, RT_HIT_TRIANGLE = 0, 1, 2
assert RAY.itemsize == 32 and HIT.itemsize == 64
# feature buffers (rt_render_aov): the two planes and the state of their accumulation
RT_AOV_ALBEDO, RT_AOV_NORMAL_DEPTH, RT_AOV_COUNT = 0, 1, 2
AOV_INFO = np.dtype([("framesAccumulated", "<i4"), ("lastSampleLanes", "<i4"), ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
# denoiser (rt_denoise): the parameters of a call and the state of the last one
DENOISE_PARAMS = np.dtype([("iterations", "<i4"), ("demodulate", "<i4"), ("sigmaColour", "<f4"), ("sigmaNormal", "<f4"), ("sigmaDepth", "<f4"),
                           ("_reserved", "<i4", 3)])
DENOISE_INFO = np.dtype([("iterations", "<i4"), ("demodulate", "<i4"), ("width", "<i4"), ("height", "<i4"),
                         ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert DENOISE_PARAMS.itemsize == 32 and DENOISE_INFO.itemsize == 32
# temporal reprojection (rt_temporal): the parameters of a call and the state of the step
TEMPORAL_PARAMS = np.dtype([("maxHistory", "<i4"), ("depthTolerance", "<f4"), ("normalTolerance", "<f4"), ("_reserved", "<i4", 5)])
TEMPORAL_INFO = np.dtype([("calls", "<i4"), ("width", "<i4"), ("height", "<i4"), ("_reserved", "<i4"),
                          ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert TEMPORAL_PARAMS.itemsize == 32 and TEMPORAL_INFO.itemsize == 32
# variance-guided denoiser (rt_denoise_variance): the parameters of a call and the state of the last one
VDENOISE_PARAMS = np.dtype([("iterations", "<i4"), ("demodulate", "<i4"), ("source", "<i4"), ("sigmaLuminance", "<f4"), ("sigmaNormal", "<f4"),
                            ("sigmaDepth", "<f4"), ("_reserved", "<i4", 2)])
VDENOISE_INFO = np.dtype([("iterations", "<i4"), ("source", "<i4"), ("width", "<i4"), ("height", "<i4"),
                          ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert VDENOISE_PARAMS.itemsize == 32 and VDENOISE_INFO.itemsize == 32
# radiance queries (rt_trace_radiance): the parameters of a call and the state of the last one
RADIANCE_PARAMS = np.dtype([("samples", "<i4"), ("seed", "<u4"), ("firstIndex", "<u4"), ("_reserved", "<i4", 5)])
RADIANCE_INFO = np.dtype([("samples", "<i4"), ("lastSampleLanes", "<i4"), ("calls", "<i4"), ("_reserved", "<i4"),
                          ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert RADIANCE_PARAMS.itemsize == 32 and RADIANCE_INFO.itemsize == 32
# gather queries (rt_gather): the parameters of a call and the state of the last one
GATHER_COSINE, GATHER_SH9 = 0, 1
GATHER_PARAMS = np.dtype([("samples", "<i4"), ("seed", "<u4"), ("firstIndex", "<u4"), ("mode", "<i4"), ("_reserved", "<i4", 4)])
GATHER_INFO = np.dtype([("samples", "<i4"), ("lastSampleLanes", "<i4"), ("calls", "<i4"), ("mode", "<i4"),
                        ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert GATHER_PARAMS.itemsize == 32 and GATHER_INFO.itemsize == 32
# visibility gathers (rt_visibility): the parameters of a call and the state of the last one
VIS_COSINE, VIS_SH9, VIS_DISTANCE = 0, 1, 2
VISIBILITY_DEFAULT_SAMPLES = 64          # RT_VISIBILITY_DEFAULT_SAMPLES of include/rt.h (what a null rt_visibility_params means)
VISIBILITY_PARAMS = np.dtype([("samples", "<i4"), ("seed", "<u4"), ("firstIndex", "<u4"), ("mode", "<i4"), ("_reserved", "<i4", 4)])
VISIBILITY_INFO = np.dtype([("samples", "<i4"), ("lastSampleLanes", "<i4"), ("calls", "<i4"), ("mode", "<i4"),
                            ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8")])
assert VISIBILITY_PARAMS.itemsize == 32 and VISIBILITY_INFO.itemsize == 32
# closest-point queries (rt_closest_points): the record of a point's nearest surface and the state of the last call
CLOSEST = np.dtype([("dst", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("kind", "<i4"), ("primitive", "<i4"), ("chunk", "<i4"),
                    ("mesh", "<i4"), ("u", "<f4"), ("v", "<f4"), ("side", "<i4"), ("_reserved", "<i4", 2)])
CLOSEST_INFO = np.dtype([("calls", "<i4"), ("_reserved", "<i4"), ("lastKernelMs", "<f8"), ("totalKernelMs", "<f8"),
                         ("lastNodeSteps", "<u8"), ("lastPrimTests", "<u8")])
assert CLOSEST.itemsize == 64 and CLOSEST_INFO.itemsize == 40
# multi-hit ray queries (rt_trace_hits): the params of a call, one of a ray's K records, and the state of the last call
HITS_PARAMS = np.dtype([("maxHits", "<i4"), ("mode", "<i4"), ("countAll", "<i4"), ("_reserved", "<i4", 5)])
MULTIHIT = np.dtype([("dst", "<f4"), ("hitPoint", "<f4", 3), ("normal", "<f4", 3), ("kind", "<i4"), ("primitive", "<i4"), ("chunk", "<i4"),
                     ("mesh", "<i4"), ("u", "<f4"), ("v", "<f4"), ("side", "<i4"), ("hitCount", "<i4"), ("_reserved", "<i4")])
HITS_INFO = np.dtype([("calls", "<i4"), ("lastMaxHits", "<i4"), ("lastMode", "<i4"), ("lastCountAll", "<i4"), ("lastKernelMs", "<f8"),
                      ("totalKernelMs", "<f8")])
assert HITS_PARAMS.itemsize == 32 and MULTIHIT.itemsize == 64 and HITS_INFO.itemsize == 32
HITS_FRONT, HITS_BOTH, HITS_MAX, HITS_DEFAULT_MAX = 0, 1, 8, 4      # RT_HITS_* of include/rt.h
assert MATERIAL.itemsize == 64 and SPHERE.itemsize == 80 and TRIANGLE.itemsize == 72 and MESHINFO.itemsize == 96

# RT_DENOISE_DEFAULT_* of include/rt.h (what a null rt_denoise_params means)
DENOISE_DEFAULTS = {"iterations": 5, "demodulate": 0, "sigmaColour": 16.0, "sigmaNormal": 1.0, "sigmaDepth": 0.5}
# RT_TEMPORAL_DEFAULT_* of include/rt.h (what a null rt_temporal_params means)
TEMPORAL_DEFAULTS = {"maxHistory": 32, "depthTolerance": 0.05, "normalTolerance": 0.5}
# RT_VDENOISE_DEFAULT_* of include/rt.h (what a null rt_vdenoise_params means; source 0)
VDENOISE_DEFAULTS = {"iterations": 3, "demodulate": 1, "source": 0, "sigmaLuminance": 8.0, "sigmaNormal": 0.25, "sigmaDepth": 0.5}

RT_INTERSECT_FLAT_CHUNKS = 0
RT_INTERSECT_BRUTE = 1

# every record rt_sizeof knows, beside its layout here (load_library checks each size against the library's)
_RECORDS = {
    "rt_material": MATERIAL, "rt_sphere": SPHERE, "rt_triangle": TRIANGLE, "rt_meshinfo": MESHINFO, "rt_params": PARAMS, "rt_stats": STATS,
    "rt_mesh_transform": MESH_TRANSFORM, "rt_local_chunk": LOCAL_CHUNK, "rt_multi_info": MULTI_INFO,
    "rt_ray": RAY, "rt_hit": HIT, "rt_aov_info": AOV_INFO,
    "rt_denoise_params": DENOISE_PARAMS, "rt_denoise_info": DENOISE_INFO, "rt_temporal_params": TEMPORAL_PARAMS, "rt_temporal_info": TEMPORAL_INFO,
    "rt_vdenoise_params": VDENOISE_PARAMS, "rt_vdenoise_info": VDENOISE_INFO, "rt_radiance_params": RADIANCE_PARAMS, "rt_radiance_info": RADIANCE_INFO,
    "rt_gather_params": GATHER_PARAMS, "rt_gather_info": GATHER_INFO, "rt_visibility_params": VISIBILITY_PARAMS, "rt_visibility_info": VISIBILITY_INFO,
    "rt_closest": CLOSEST, "rt_closest_info": CLOSEST_INFO, "rt_hits_params": HITS_PARAMS, "rt_multihit": MULTIHIT, "rt_hits_info": HITS_INFO,
}

# ---- the signatures of include/rt.h: C entry -> (argtypes, or None where none are set; restype) ------------------------
_V, _I, _Z, _F, _S = c_void_p, c_int, c_size_t, POINTER(c_float), c_char_p      # _V: a handle or any other pointer
_SIGNATURES = {}


def _declare(argtypes, names, restype=c_int):
    for n in names.split():
        _SIGNATURES[n] = (argtypes, restype)


def _families(*stems):
    """the three entries of each query family: a context's on host arrays, its _device twin, and the multi handle's"""
    return " ".join(f"rt_{s} rt_{s}_device rt_multi_{s}" for s in stems)


_declare([_V], "rt_reset_accum rt_wait rt_reset_aov rt_reset_temporal rt_multi_count rt_multi_reset_accum rt_multi_reset_aov rt_multi_reset_temporal")
_declare([_V], "rt_destroy rt_multi_destroy", None)
_declare([_V], "rt_last_error rt_multi_last_error", c_char_p)
_declare([_V, _I], "rt_render_frame rt_render_frame_flat rt_submit_frame")
_declare([_V, _I], "rt_multi_context", c_void_p)
_declare([_V, _I, _I], "rt_set_rows rt_set_bands rt_render rt_render_counting rt_render_aov rt_multi_render rt_multi_render_aov")
_declare([_V, _V], "rt_set_stream rt_set_params rt_multi_set_params "                                   # (handle, a record or a stream)
         "rt_get_stats rt_get_aov_info rt_get_denoise_info rt_get_temporal_info rt_get_vdenoise_info rt_get_radiance_info rt_get_gather_info "
         "rt_get_visibility_info rt_get_closest_info rt_get_hits_info rt_multi_get_info "
         "rt_denoise rt_temporal rt_denoise_temporal rt_denoise_variance "
         "rt_multi_denoise rt_multi_temporal rt_multi_denoise_temporal rt_multi_denoise_variance")
_declare([_V, _V, _I], "rt_upload_spheres rt_upload_triangles rt_upload_meshinfo rt_set_mesh_transforms "   # (handle, records, count)
         "rt_multi_upload_spheres rt_multi_upload_triangles rt_multi_upload_meshinfo rt_multi_set_mesh_transforms")
_declare([_V, _F, _Z], "rt_read_accum rt_read_last_frame rt_read_denoised rt_read_temporal rt_read_temporal_history rt_read_variance "
         "rt_multi_read_accum rt_multi_read_denoised rt_multi_read_temporal rt_multi_read_temporal_history rt_multi_read_variance")
_declare([_V, _V, _Z], "rt_read_display rt_read_denoised_display rt_read_temporal_display rt_read_bvh_order "
         "rt_copy_accum_to_device rt_copy_denoised_to_device rt_copy_temporal_to_device rt_copy_variance_to_device "
         "rt_multi_read_display rt_multi_read_denoised_display rt_multi_read_temporal_display")
_declare([_V, _V, _I, _V], _families("trace_rays", "occluded", "closest_points"))                       # (handle, items, n, out)
_declare([_V, _V, _I, _V, _V], _families("trace_radiance", "gather", "visibility", "trace_hits"))       # (handle, items, n, params, out)
_declare([_I], "rt_create", c_void_p)
_declare([POINTER(c_int), _I], "rt_multi_create", c_void_p)
_declare(None, "rt_abi_version")
_declare([_S], "rt_sizeof")
_declare([_V, _S, _I], "rt_set_option rt_multi_set_option")
_declare([_V, _V, _I, _V, _I, _I], "rt_upload_local_meshes rt_multi_upload_local_meshes")
_declare([_V, _V, _I, _V, _I], "rt_read_world_geometry")
_declare([_V, _I, _I, _V], "rt_render_params rt_multi_render_params")
_declare([_V, _I, _V], "rt_submit_frame_params")
_declare([_V, _V, _V, _Z], "rt_read_bvh")
_declare([_V, _V, _V], "rt_multi_get_stats")
_declare([_V, _F, _Z, _I], "rt_write_accum rt_multi_write_accum")
_declare([_V, _I, _F, _Z], "rt_read_aov rt_multi_read_aov")
_declare([_V, _I, _V, _Z], "rt_copy_aov_to_device")

# every symbol include/rt.h declares (tests check that the built library exports each one)
SYMBOLS = list(_SIGNATURES)

_lib = None


class RtError(RuntimeError):
    pass


def load_library() -> ctypes.CDLL:
    """Load librt_mi355x.so (built in-tree by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError(f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                      "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in _SIGNATURES.items():
        f = getattr(lib, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    for name, dt in _RECORDS.items():
        got = lib.rt_sizeof(name.encode())
        if got != dt.itemsize:
            raise RtError(f"ABI mismatch: sizeof({name}) = {got} in the library, {dt.itemsize} in the binding")
    _lib = lib
    return lib


def _ptr(a):
    """a numpy array or record as a void* argument; None stays None (the library's defaults)"""
    return None if a is None else a.ctypes.data_as(c_void_p)


def _params_run(params):
    """a C-contiguous array of PARAMS records (one per frame) and its length"""
    p = np.ascontiguousarray(params, dtype=PARAMS).reshape(-1)
    return p, int(p.shape[0])


def _ray_array(rays) -> np.ndarray:
    """a C-contiguous RAY array from a RAY array or a float32 (n, 8) array (origin, tMax, direction, -)"""
    a = np.asarray(rays)
    if a.dtype == RAY:
        return np.ascontiguousarray(a.reshape(-1))
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"rays: a RAY array or float32 (n, 8), not {a.dtype} {a.shape}")
    return a.view(RAY).reshape(-1)


def _hits_params(max_hits, both_sides, count_all):
    """a HITS_PARAMS record"""
    p = np.zeros((), HITS_PARAMS)
    p["maxHits"], p["mode"], p["countAll"] = int(max_hits), HITS_BOTH if both_sides else HITS_FRONT, int(bool(count_all))
    return p


def _radiance_params(samples, seed, first_index):
    """None (the library's defaults: the context's numRaysPerPixel samples, seed 0, firstIndex 0) when samples is None; else a
    RADIANCE_PARAMS record"""
    if samples is None:
        if seed or first_index:
            raise TypeError("trace_radiance: seed and first_index need samples")
        return None
    p = np.zeros((), RADIANCE_PARAMS)
    p["samples"], p["seed"], p["firstIndex"] = int(samples), int(seed) & 0xFFFFFFFF, int(first_index) & 0xFFFFFFFF
    return p


def _gather_params(samples, seed, first_index, mode, default_samples=None):
    """None (the library's defaults: the context's numRaysPerPixel samples, seed 0, firstIndex 0, mode 0) when nothing is given; else a
    GATHER_PARAMS record, samples None standing for default_samples (the numRaysPerPixel of the params the caller set last)"""
    if samples is None:
        if not (seed or first_index or mode):
            return None
        if default_samples is None:
            raise TypeError("gather: samples=None with a seed, first_index or mode needs set_params first")
        samples = default_samples
    p = np.zeros((), GATHER_PARAMS)
    p["samples"], p["seed"], p["firstIndex"], p["mode"] = int(samples), int(seed) & 0xFFFFFFFF, int(first_index) & 0xFFFFFFFF, int(mode)
    return p


def _gather_shape(n, params):
    """(n, 4) in mode 0, (n, 9, 4) in mode 1"""
    return (n, 9, 4) if params is not None and int(params["mode"]) == GATHER_SH9 else (n, 4)


def _visibility_params(samples, seed, first_index, mode):
    """None (the library's defaults: 64 samples, seed 0, firstIndex 0, mode 0) when nothing is given; else a VISIBILITY_PARAMS record,
    samples None standing for the library's default count"""
    if samples is None and not (seed or first_index or mode):
        return None
    p = np.zeros((), VISIBILITY_PARAMS)
    p["samples"] = VISIBILITY_DEFAULT_SAMPLES if samples is None else int(samples)
    p["seed"], p["firstIndex"], p["mode"] = int(seed) & 0xFFFFFFFF, int(first_index) & 0xFFFFFFFF, int(mode)
    return p


def _visibility_shape(n, params):
    """(n, 4) in modes 0 and 2, (n, 12) in mode 1"""
    return (n, 12) if params is not None and int(params["mode"]) == VIS_SH9 else (n, 4)


def _hits_shape(n, params):
    return (n, int(params["maxHits"]))


def _hits_check(entry, params):
    """max_hits outside 1..HITS_MAX is refused here, under the name of the entry it was meant for, before any call"""
    K = int(params["maxHits"])
    if not 1 <= K <= HITS_MAX:
        raise RtError(f"{entry}: max_hits = {K} outside 1..{HITS_MAX}")


# The seven query families: entry stem -> (takes a params record, the host output's dtype, its shape from (n, params) — None: (n,) —,
# a check of the params that runs before any call, or None).  On a CUDA tensor the output is a tensor of the same shape and dtype, a
# record (HIT, CLOSEST, MULTIHIT) unfolded into a last axis of its 16 float32 words.  _QUERIES holds each family under the names of
# its two host entries, rt_<stem> and rt_multi_<stem>; a context's device entry is rt_<stem>_device.
_F32 = np.dtype(np.float32)
_FAMILIES = {
    "trace_rays": (False, HIT, None, None),
    "occluded": (False, np.dtype(np.uint8), None, None),
    "trace_radiance": (True, _F32, lambda n, p: (n, 4), None),
    "gather": (True, _F32, _gather_shape, None),
    "visibility": (True, _F32, _visibility_shape, None),
    "closest_points": (False, CLOSEST, None, None),
    "trace_hits": (True, MULTIHIT, _hits_shape, _hits_check),
}
_QUERIES = {prefix + stem: family for stem, family in _FAMILIES.items() for prefix in ("rt_", "rt_multi_")}

# the image filters' keyword arguments: (params record, the defaults of include/rt.h, the name a TypeError speaks of)
_DENOISE = (DENOISE_PARAMS, DENOISE_DEFAULTS, "denoise")
_TEMPORAL = (TEMPORAL_PARAMS, TEMPORAL_DEFAULTS, "temporal")
_VDENOISE = (VDENOISE_PARAMS, VDENOISE_DEFAULTS, "denoise_variance")


def _filter_params(kind, params: dict):
    """None (the library's defaults) when no field is given; else a record of the kind's dtype: the defaults of include/rt.h with the
    given fields replaced.  kind: _DENOISE, _TEMPORAL or _VDENOISE"""
    if not params:
        return None
    dtype, defaults, what = kind
    p = np.zeros((), dtype)
    for k, v in defaults.items():
        p[k] = v
    for k, v in params.items():
        if k not in defaults:
            raise TypeError(f"{what}: unknown parameter {k!r} (one of {sorted(defaults)})")
        p[k] = v
    return p


def _as_buffer(arr, dtype):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return a, a.ctypes.data_as(c_void_p), int(a.shape[0]) if a.ndim else 0


def _is_tensor(x) -> bool:
    t = type(x)
    return t.__module__.startswith("torch") and t.__name__ == "Tensor" and getattr(x, "is_cuda", False)


def _device_triangles(tris, n):
    """(device pointer, count, torch device or None) of upload_triangles_device's arguments"""
    if _is_tensor(tris):
        import torch
        if tris.dtype != torch.float32 or tris.dim() != 2 or tris.shape[1] != 18 or not tris.is_contiguous():
            raise ValueError(f"triangles: a contiguous float32 (n, 18) CUDA tensor, not {tris.dtype} {tuple(tris.shape)}")
        if n is not None and int(n) != int(tris.shape[0]):
            raise ValueError(f"n = {n} for a tensor of {int(tris.shape[0])} triangles")
        return int(tris.data_ptr()), int(tris.shape[0]), tris.device
    if isinstance(tris, (int, np.integer)) and not isinstance(tris, bool):
        if n is None:
            raise ValueError("a device pointer needs n")
        return int(tris), int(n), None
    raise ValueError("triangles: a float32 (n, 18) CUDA tensor, or an int device pointer and n")


def _arm_device_geometry(tracer):
    """option "device_geometry" for an upload from device memory: set to 1 unless set_option has set it; set to 0 it refuses here"""
    state = getattr(tracer, "_device_geometry", None)
    if state is None:
        tracer.set_option("device_geometry", 1)
    elif state == 0:
        raise RtError("upload_triangles_device: option device_geometry is 0 (a device pointer would be read as host memory)")


class _Handle:
    """What a Tracer (an rt_ctx, entries rt_*) and a MultiTracer (an rt_multi, entries rt_multi_*) share: the library, the handle and its
    life, the checked call, and one helper for each kind of entry — plane, display and info readers, copies to device memory, filters
    with an optional params record, uploads and the query families."""

    _PREFIX = None                  # "rt_" or "rt_multi_": the handle's create, destroy, last_error, set_option and upload entries
    _DEVICE_ENTRIES = False         # whether the query families have _device entries for CUDA tensors (a context's do)
    _closest_k = 1                  # option "closest_k" as this handle's set_option set it last: the records closest_points allocates per
                                    # point.  The option must be set through the handle: set behind its back (the raw library, another
                                    # host on the same rt_ctx) the C call would write K records per point into a buffer of one per point
    # per instance: _lib, _handle, and _params — the PARAMS set last, once there are any (the default sample count of gather)

    def _open(self, *args):
        self._lib = load_library()
        self._handle = getattr(self._lib, self._PREFIX + "create")(*args)
        if not self._handle:
            raise RtError(f"{self._PREFIX}create failed: " + (getattr(self._lib, self._PREFIX + "last_error")(None) or b"").decode())

    def close(self):
        if getattr(self, "_handle", None):
            getattr(self._lib, self._PREFIX + "destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise RtError(f"{what} failed ({rc}): " + (getattr(self._lib, self._PREFIX + "last_error")(self._handle) or b"").decode())

    def _call(self, name, *args):
        """The C entry `name` on this handle, checked.  For entries that come with buffers to prepare or results to unpack; the entries
        that only pass a few ints and may be called every frame (render*, submit_frame, wait, reset_*, set_rows, set_bands) write
        self._check(self._lib.<entry>(self._handle, ...), "<entry>") out instead: forwarding *args costs such a call 0.12 us, a
        third of all it takes (profiles/cabi_refactor_overhead.txt)."""
        rc = getattr(self._lib, name)(self._handle, *args)
        if rc != 0:
            self._check(rc, name)

    def _set_option(self, name, value):
        entry = self._PREFIX + "set_option"
        self._check(getattr(self._lib, entry)(self._handle, name.encode(), int(value)), f"{entry}({name})")
        if name == "device_geometry":
            self._device_geometry = int(value)
        elif name == "closest_k":
            self._closest_k = int(value)        # (records per point of closest_points: the shape of its result)

    def _upload(self, spheres, triangles, meshinfo):
        for arr, dt, what in ((spheres, SPHERE, "spheres"), (triangles, TRIANGLE, "triangles"), (meshinfo, MESHINFO, "meshinfo")):
            if arr is not None:
                a, ptr, n = _as_buffer(arr, dt)
                self._call(f"{self._PREFIX}upload_{what}", ptr, n)

    # The helpers below fetch their entry and test its result themselves: a second *args frame under each costs a call that does little
    # else a tenth of a microsecond and more (profiles/cabi_refactor_overhead.txt).

    def _plane(self, name, shape, which=None):
        """a plane reader: float32 of `shape` filled by `name`(handle, [which,] float*, size)"""
        out = np.empty(shape, np.float32)
        entry, ptr = getattr(self._lib, name), out.ctypes.data_as(_F)
        rc = entry(self._handle, ptr, out.size) if which is None else entry(self._handle, which, ptr, out.size)
        if rc != 0:
            self._check(rc, name)
        return out

    def _display(self, name, shape):
        """a display reader: one packed sRGB RGBA8 word per pixel of `shape`, returned as uint8 (*shape, 4)"""
        out = np.empty(shape, np.uint32)
        rc = getattr(self._lib, name)(self._handle, out.ctypes.data_as(c_void_p), out.size)
        if rc != 0:
            self._check(rc, name)
        return out.view(np.uint8).reshape(*shape, 4)

    def _to_device(self, name, device_ptr, n_floats, *first):
        self._call(name, *first, c_void_p(device_ptr), n_floats)

    def _record(self, name, dtype, *more):
        """a zeroed record of `dtype` filled by `name`(handle, record*, *more), as a dict of its fields"""
        s = np.zeros((), dtype)
        self._call(name, _ptr(s), *more)
        return {k: (s[k].item() if s[k].ndim == 0 else s[k].tolist()) for k in dtype.names}

    def _info(self, name, dtype):
        """an *_info reader: the record's fields without its padding word `_reserved` (stats() is no info reader: it returns STATS whole,
        `_reserved` included, as it always has)"""
        d = self._record(name, dtype)
        d.pop("_reserved", None)
        return d

    def _filter(self, name, kind, params):
        """an image filter: `name`(handle, params record or NULL), the record made of the keywords `params` as _filter_params does"""
        p = _filter_params(kind, params) if params else None            # (no keywords, the common call: not worth a frame)
        rc = getattr(self._lib, name)(self._handle, None if p is None else p.ctypes.data_as(c_void_p))
        if rc != 0:
            self._check(rc, name)

    def _gather_params(self, samples, seed, first_index, mode):
        last = getattr(self, "_params", None)
        return _gather_params(samples, seed, first_index, mode, None if last is None else int(last["numRaysPerPixel"]))

    def _query(self, name, items, params=None):
        """A query family of _QUERIES: its host entry `name` on arrays (items as _ray_array takes them; the output zero-initialised), and
        on a handle with device entries `name`_device on a float32 CUDA tensor (n, 8) of the context's device, ordered with torch's
        current stream as _on_torch_stream describes."""
        takes_params, dtype, shape, check = _QUERIES[name]
        tensor = self._DEVICE_ENTRIES and _is_tensor(items)
        if tensor:
            name += "_device"
        items = self._ray_tensor(items) if tensor else _ray_array(items)
        n = int(items.shape[0])
        if check is not None:
            check(name, params)
        shape = (n,) if shape is None else shape(n, params)
        if dtype is CLOSEST and self._closest_k != 1:
            shape += (self._closest_k,)         # K-nearest queries (option "closest_k"): K records per point
        entry, qp = getattr(self._lib, name), None if params is None else params.ctypes.data_as(c_void_p)
        if tensor:
            import torch
            out = torch.empty(shape + (dtype.itemsize // 4,) if dtype.names else shape, dtype=torch.uint8 if dtype == np.uint8 else torch.float32,
                              device=items.device)
            src, dst = c_void_p(items.data_ptr()), c_void_p(out.data_ptr())
            call = (lambda: entry(self._handle, src, n, qp, dst)) if takes_params else (lambda: entry(self._handle, src, n, dst))
            self._on_torch_stream(items.device, call, name)
            return out
        out = np.zeros(shape, dtype)
        src, dst = items.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p)
        rc = entry(self._handle, src, n, qp, dst) if takes_params else entry(self._handle, src, n, dst)
        if rc != 0:
            self._check(rc, name)
        return out


class Tracer(_Handle):
    """One rt_ctx.  Thin, exception-raising wrapper; semantics are those documented in include/rt.h."""

    _PREFIX, _DEVICE_ENTRIES = "rt_", True
    _ctx = property(lambda self: self._handle, lambda self, h: setattr(self, "_handle", h))

    def __init__(self, device: int = 0):
        self._open(device)

    # -- uploads
    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._params = p.copy()
        self._call("rt_set_params", _ptr(p))

    def upload(self, spheres=None, triangles=None, meshinfo=None):
        self._upload(spheres, triangles, meshinfo)

    def upload_triangles_device(self, tris, n=None):
        """rt_upload_triangles from device memory (option "device_geometry", which this sets to 1 unless set_option has set it): a
        contiguous float32 CUDA tensor (n, 18) on the context's device — the copy is ordered with torch's current stream as trace_rays'
        device entry is, so the tensor may be overwritten on that stream right after the call — or an int device pointer and n, copied on
        the context's stream.  With the option set to 0 this raises before anything is called: a device pointer never reaches the host
        path."""
        tensor = _is_tensor(tris)
        ptr, n, device = _device_triangles(tris, n)
        _arm_device_geometry(self)
        call = lambda: self._lib.rt_upload_triangles(self._handle, c_void_p(ptr), n)      # noqa: E731
        if tensor:
            self._on_torch_stream(device, call, "rt_upload_triangles")
        else:
            self._check(call(), "rt_upload_triangles")

    # -- on-device geometry pipeline
    def upload_local_meshes(self, local_tris, chunks, n_meshes: int):
        t, tp, nt = _as_buffer(local_tris, TRIANGLE)
        ch, cp, nc = _as_buffer(chunks, LOCAL_CHUNK)
        self._local_counts = (nt, nc)
        self._call("rt_upload_local_meshes", tp, nt, cp, nc, int(n_meshes))

    def set_mesh_transforms(self, transforms):
        x, xp, n = _as_buffer(transforms, MESH_TRANSFORM)
        self._call("rt_set_mesh_transforms", xp, n)

    def read_world_geometry(self):
        nt, nc = self._local_counts
        tris, infos = np.zeros(nt, TRIANGLE), np.zeros(nc, MESHINFO)
        self._call("rt_read_world_geometry", _ptr(tris), nt, _ptr(infos), nc)
        return tris, infos

    def set_rows(self, row0: int, nrows: int):
        self._rows = (row0, nrows)
        self._check(self._lib.rt_set_rows(self._handle, row0, nrows), "rt_set_rows")

    def set_bands(self, first_band: int, band_stride: int, height: int = None):
        H = int(self._params["height"]) if height is None else height
        self._rows = (first_band * 8, sum(min(8, H - y) for y in range(first_band * 8, H, band_stride * 8)))
        self._check(self._lib.rt_set_bands(self._handle, first_band, band_stride), "rt_set_bands")

    def set_option(self, name: str, value: int):
        self._set_option(name, value)

    def set_stream(self, stream_ptr):
        self._call("rt_set_stream", c_void_p(stream_ptr))
        self._stream = stream_ptr

    # -- ray queries
    def trace_rays(self, rays):
        """rt_trace_rays: the closest hit of every ray.  rays: a RAY array or float32 (n, 8) -> a HIT array.  A float32 CUDA tensor
        (n, 8) on the context's device takes the device entry instead and returns a float32 (n, 16) tensor (the HIT records)."""
        return self._query("rt_trace_rays", rays)

    def occluded(self, rays):
        """rt_occluded: 1 where the closest-hit query of the ray would hit.  rays as for trace_rays -> uint8 (n,) (array or tensor)."""
        return self._query("rt_occluded", rays)

    @staticmethod
    def _ray_tensor(rays):
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays: a float32 (n, 8) tensor, not {rays.dtype} {tuple(rays.shape)}")
        return rays.contiguous()

    def _on_torch_stream(self, device, call, what):
        """call() — a device entry — ordered with torch's current stream of `device`.

        The device entries on torch tensors, ordered with torch's current stream both ways: the context runs the call on that stream
        (rt_set_stream: the stream first waits for what the context enqueued before) and goes back to its own stream (or the one set_stream
        gave it) afterwards, which then waits for the query (rt_set_stream's switch is ordered) — so torch's later work on the stream sees
        the results, and the context's next upload, geometry pass or render cannot overtake the query.  torch's legacy default stream has no handle the
        library can take (NULL means the context's own stream), so there the call is fenced: torch's stream is synchronised before it and
        the device after it.  (torch ships its own HIP runtime: import torch before the library is loaded, so that both use that one.)"""
        import torch
        stream = torch.cuda.current_stream(device)
        handle = int(stream.cuda_stream)
        if handle == 0:
            stream.synchronize()
            rc = call()
            torch.cuda.synchronize(device)
            self._check(rc, what)
            return
        self._check(self._lib.rt_set_stream(self._handle, c_void_p(handle)), "rt_set_stream")
        try:
            rc = call()
        finally:
            self._lib.rt_set_stream(self._handle, c_void_p(getattr(self, "_stream", None) or None))
        self._check(rc, what)

    # -- radiance queries
    def trace_radiance(self, rays, samples=None, seed=0, first_index=0):
        """rt_trace_radiance: Trace along every ray, averaged over `samples` runs (None: the context's numRaysPerPixel, seed 0, first
        index 0).  rays: a RAY array or float32 (n, 8) -> float32 (n, 4).  A float32 CUDA tensor (n, 8) on the context's device takes the
        device entry, ordered with torch's current stream as trace_rays is, and returns a float32 (n, 4) tensor."""
        return self._query("rt_trace_radiance", rays, _radiance_params(samples, seed, first_index))

    def radiance_info(self) -> dict:
        return self._info("rt_get_radiance_info", RADIANCE_INFO)

    # -- gather queries
    def gather(self, points, samples=None, seed=0, first_index=0, mode=GATHER_COSINE):
        """rt_gather: the light arriving at every point over `samples` directions drawn on the device (None: the context's
        numRaysPerPixel, seed 0, first index 0, mode 0).  points: a RAY array or float32 (n, 8) — origin, tMax, NORMAL, - .  mode
        GATHER_COSINE -> float32 (n, 4), the mean radiance over the cosine lobe (irradiance = pi times it); GATHER_SH9 -> float32
        (n, 9, 4), the SH coefficients of the incoming radiance.  A float32 CUDA tensor (n, 8) on the context's device takes the device
        entry, ordered with torch's current stream as trace_rays is, and returns a tensor of that shape.  samples=None with a seed, first
        index or mode (gather(points, mode=GATHER_SH9)) is the numRaysPerPixel of the params set last, as the library's own default is."""
        return self._query("rt_gather", points, self._gather_params(samples, seed, first_index, mode))

    def gather_info(self) -> dict:
        return self._info("rt_get_gather_info", GATHER_INFO)

    # -- visibility gathers
    def visibility(self, points, samples=None, seed=0, first_index=0, mode=VIS_COSINE):
        """rt_visibility: how open every point is over `samples` directions drawn on the device — rt_gather's directions, bit for bit
        (None: 64 samples).  points: a RAY array or float32 (n, 8) — origin, the reach tMax, NORMAL, - .  No params are needed.  mode
        VIS_COSINE -> float32 (n, 4): the bent normal (the mean open direction, not normalised) and the visibility fraction (ambient
        occlusion = 1 - it); VIS_SH9 -> float32 (n, 12): nine SH coefficients of the visibility function, the visibility fraction, 0, 0;
        VIS_DISTANCE -> float32 (n, 4): mean distance (a miss counts the reach), mean squared distance, hit fraction, 1.  A float32 CUDA
        tensor (n, 8) on the context's device takes the device entry, ordered with torch's current stream as trace_rays is, and returns a
        tensor of that shape."""
        return self._query("rt_visibility", points, _visibility_params(samples, seed, first_index, mode))

    visibility_device = visibility          # (a tensor takes rt_visibility_device; the name says so at the call site)

    def visibility_info(self) -> dict:
        return self._info("rt_get_visibility_info", VISIBILITY_INFO)

    # -- closest-point queries
    def closest_points(self, points):
        """rt_closest_points: the nearest sphere or triangle to every point, where on it, how far and on which side.  points: a RAY array
        or float32 (n, 8) — the point, the search radius in tMax (inf: unbounded), the rest unread -> a CLOSEST array.  No params are
        needed.  A float32 CUDA tensor (n, 8) on the context's device takes the device entry, ordered with torch's current stream as
        trace_rays is, and returns a float32 (n, 16) tensor (the CLOSEST records)."""
        # (after set_option("closest_k", K) with K > 1 every point gets K records, nearest first — include/rt.h "K-nearest queries",
        # nearest.py: a CLOSEST array (n, K), a tensor (n, K, 16); _query adds the axis)
        return self._query("rt_closest_points", points)

    closest_points_device = closest_points  # (a tensor takes rt_closest_points_device; the name says so at the call site)

    def closest_info(self) -> dict:
        return self._info("rt_get_closest_info", CLOSEST_INFO)

    # -- multi-hit ray queries
    def trace_hits(self, rays, max_hits=HITS_DEFAULT_MAX, both_sides=False, count_all=False):
        """rt_trace_hits: the first max_hits (1..8) surfaces along every ray, nearest first.  rays: a RAY array or float32 (n, 8) -> a
        MULTIHIT array (n, max_hits); records past a ray's last hit are empty (kind 0, dst inf).  both_sides: back faces of triangles
        and the exit points of spheres count too (side = -1).  count_all: hitCount is the number of all hits below tMax instead of
        min(hits, max_hits).  No params are needed.  A float32 CUDA tensor (n, 8) on the context's device takes the device entry,
        ordered with torch's current stream as trace_rays is, and returns a float32 (n, max_hits, 16) tensor (the MULTIHIT records)."""
        return self._query("rt_trace_hits", rays, _hits_params(max_hits, both_sides, count_all))

    trace_hits_device = trace_hits  # (a tensor takes rt_trace_hits_device; the name says so at the call site)

    def hits_info(self) -> dict:
        return self._info("rt_get_hits_info", HITS_INFO)

    # -- rendering
    def render_frame(self, frame: int):
        self._check(self._lib.rt_render_frame(self._handle, frame), "rt_render_frame")

    def render(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_render(self._handle, first_frame, n_frames), "rt_render")

    def render_params(self, first_frame: int, params):
        """rt_render_params: frame first_frame + f with the uniforms params[f] (a PARAMS array; all entries share the settings)."""
        p, n = _params_run(params)
        self._call("rt_render_params", int(first_frame), n, _ptr(p))
        if n:
            self._params = p[-1].copy()

    def render_counting(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_render_counting(self._handle, first_frame, n_frames), "rt_render_counting")

    def render_frame_flat(self, frame: int):
        self._check(self._lib.rt_render_frame_flat(self._handle, frame), "rt_render_frame_flat")

    def reset_accum(self):
        self._check(self._lib.rt_reset_accum(self._handle), "rt_reset_accum")

    # -- read-back
    def _strip_shape(self):
        W, H = int(self._params["width"]), int(self._params["height"])
        rows = getattr(self, "_rows", (0, H))[1]
        return rows, W

    def _image_shape(self):
        return int(self._params["height"]), int(self._params["width"])

    def read_accum(self) -> np.ndarray:
        return self._plane("rt_read_accum", self._strip_shape() + (4,))

    def submit_frame(self, frame_index: int):
        """Queue one frame (returns at once); wait() or any other call makes sure it is in resultTexture."""
        self._check(self._lib.rt_submit_frame(self._handle, int(frame_index)), "rt_submit_frame")

    def submit_frame_params(self, frame_index: int, params):
        """rt_submit_frame_params: queue one frame with its own uniforms (a camera move does not wait for the queue)."""
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._call("rt_submit_frame_params", int(frame_index), _ptr(p))
        self._params = p.copy()

    def wait(self):
        self._check(self._lib.rt_wait(self._handle), "rt_wait")

    def write_accum(self, rgba, frames_rendered: int):
        """Restore a saved resultTexture (as read_accum returned it) and the frame counter."""
        a = np.ascontiguousarray(rgba, np.float32)
        self._call("rt_write_accum", a.ctypes.data_as(_F), a.size, int(frames_rendered))

    def read_last_frame(self) -> np.ndarray:
        return self._plane("rt_read_last_frame", self._strip_shape() + (4,))

    def read_display(self) -> np.ndarray:
        """resultTexture as sRGB RGBA8, shape (rows, W, 4) uint8, row 0 = bottom."""
        return self._display("rt_read_display", self._strip_shape())

    def copy_accum_to_device(self, device_ptr: int, n_floats: int):
        self._to_device("rt_copy_accum_to_device", device_ptr, n_floats)

    def read_bvh(self):
        """(f32 nodes [n, 32] float32 view, f16 nodes [n, 32] uint32) of the built BVH4 (see rt_read_bvh)."""
        n = self.stats()["numBvhNodes"]
        f32, f16 = np.zeros((n, 32), np.uint32), np.zeros((n, 32), np.uint32)
        self._call("rt_read_bvh", _ptr(f32), _ptr(f16), n)
        return f32, f16

    def read_bvh_order(self):
        """BVH position -> uploaded triangle (see rt_read_bvh_order), uint32 [sum of the leaf counts of read_bvh()]."""
        refs = self.read_bvh()[0][:, 24:28].ravel()
        leaves = refs[((refs & 0x80000000) != 0) & (refs != 0xFFFFFFFF)]
        order = np.zeros(int(((leaves & 3) + 1).sum()), np.uint32)
        self._call("rt_read_bvh_order", _ptr(order), order.size)
        return order

    # -- feature buffers
    def render_aov(self, first_frame: int, n_frames: int):
        """rt_render_aov: accumulate the feature frames first_frame .. first_frame + n_frames - 1 into the two planes."""
        self._check(self._lib.rt_render_aov(self._handle, int(first_frame), int(n_frames)), "rt_render_aov")

    def read_aov(self, which: int) -> np.ndarray:
        """rt_read_aov: plane RT_AOV_ALBEDO (albedo.rgb, coverage) or RT_AOV_NORMAL_DEPTH (normal.xyz, depth) of this context's strip."""
        return self._plane("rt_read_aov", self._strip_shape() + (4,), int(which))

    def copy_aov_to_device(self, which: int, device_ptr: int, n_floats: int):
        self._to_device("rt_copy_aov_to_device", device_ptr, n_floats, int(which))

    def reset_aov(self):
        self._check(self._lib.rt_reset_aov(self._handle), "rt_reset_aov")

    def aov_info(self) -> dict:
        return self._info("rt_get_aov_info", AOV_INFO)

    # -- denoiser
    def denoise(self, **params):
        """rt_denoise: filter resultTexture, guided by the feature planes, into the denoised plane.  Keywords: iterations, demodulate,
        sigmaColour, sigmaNormal, sigmaDepth; none = the library's defaults."""
        self._filter("rt_denoise", _DENOISE, params)

    def read_denoised(self) -> np.ndarray:
        return self._plane("rt_read_denoised", self._image_shape() + (4,))

    def read_denoised_display(self) -> np.ndarray:
        """the denoised plane as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        return self._display("rt_read_denoised_display", self._image_shape())

    def copy_denoised_to_device(self, device_ptr: int, n_floats: int):
        self._to_device("rt_copy_denoised_to_device", device_ptr, n_floats)

    def denoise_info(self) -> dict:
        return self._info("rt_get_denoise_info", DENOISE_INFO)

    # -- temporal reprojection
    def temporal(self, **params):
        """rt_temporal: reproject the previous temporal colour into the current camera's view and blend resultTexture in.  Keywords:
        maxHistory, depthTolerance, normalTolerance; none = the library's defaults."""
        self._filter("rt_temporal", _TEMPORAL, params)

    def reset_temporal(self):
        self._check(self._lib.rt_reset_temporal(self._handle), "rt_reset_temporal")

    def read_temporal(self) -> np.ndarray:
        return self._plane("rt_read_temporal", self._image_shape() + (4,))

    def read_temporal_history(self) -> np.ndarray:
        """the history length N per pixel, shape (H, W)"""
        return self._plane("rt_read_temporal_history", self._image_shape())

    def read_temporal_display(self) -> np.ndarray:
        """the temporal colour as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        return self._display("rt_read_temporal_display", self._image_shape())

    def copy_temporal_to_device(self, device_ptr: int, n_floats: int):
        self._to_device("rt_copy_temporal_to_device", device_ptr, n_floats)

    def temporal_info(self) -> dict:
        return self._info("rt_get_temporal_info", TEMPORAL_INFO)

    def denoise_temporal(self, **params):
        """rt_denoise_temporal: Tracer.denoise with the temporal colour in place of resultTexture; read with read_denoised*"""
        self._filter("rt_denoise_temporal", _DENOISE, params)

    # -- variance-guided denoiser
    def denoise_variance(self, **params):
        """rt_denoise_variance: the variance-guided filter of resultTexture (source 0) or the temporal colour (source 1) into the denoised
        plane; read with read_denoised*, var_0 with read_variance.  Keywords: iterations, demodulate, source, sigmaLuminance,
        sigmaNormal, sigmaDepth; none = the library's defaults."""
        self._filter("rt_denoise_variance", _VDENOISE, params)

    def read_variance(self) -> np.ndarray:
        """var_0 of the last denoise_variance(), shape (H, W)"""
        return self._plane("rt_read_variance", self._image_shape())

    def copy_variance_to_device(self, device_ptr: int, n_floats: int):
        self._to_device("rt_copy_variance_to_device", device_ptr, n_floats)

    def vdenoise_info(self) -> dict:
        return self._info("rt_get_vdenoise_info", VDENOISE_INFO)

    def stats(self) -> dict:
        return self._record("rt_get_stats", STATS)


class MultiTracer(_Handle):
    """One rt_multi: N contexts (one per entry of `devices`; a device may repeat), interleaved 8-row bands, one gather to the
    first device at the end of render()."""

    _PREFIX = "rt_multi_"
    _m = property(lambda self: self._handle, lambda self, h: setattr(self, "_handle", h))
    _shape = None                   # (H, W) of the params set last

    def __init__(self, devices):
        self._open((c_int * len(devices))(*devices), len(devices))

    def _image_shape(self):
        H, W = self._shape              # (None before set_params: the readers fail here, before any call)
        return H, W

    def count(self) -> int:
        return self._lib.rt_multi_count(self._handle)

    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._shape = (int(p["height"]), int(p["width"]))
        self._params = p.copy()
        self._call("rt_multi_set_params", _ptr(p))

    def upload(self, spheres=None, triangles=None, meshinfo=None):
        self._upload(spheres, triangles, meshinfo)

    def upload_local_meshes(self, local_tris, chunks, n_meshes: int):
        t, tp, nt = _as_buffer(local_tris, TRIANGLE)
        ch, cp, nc = _as_buffer(chunks, LOCAL_CHUNK)
        self._call("rt_multi_upload_local_meshes", tp, nt, cp, nc, int(n_meshes))

    def set_mesh_transforms(self, transforms):
        x, xp, n = _as_buffer(transforms, MESH_TRANSFORM)
        self._call("rt_multi_set_mesh_transforms", xp, n)

    def read_display(self) -> np.ndarray:
        """the assembled resultTexture as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        return self._display("rt_multi_read_display", self._image_shape())

    def write_accum(self, rgba, frames_rendered: int):
        """Restore a saved resultTexture (the whole image, as read_accum returned it) and the frame counter on every context."""
        a = np.ascontiguousarray(rgba, np.float32)
        self._call("rt_multi_write_accum", a.ctypes.data_as(_F), a.size, int(frames_rendered))

    def set_option(self, name: str, value: int):
        self._set_option(name, value)

    def upload_triangles_device(self, tris, n=None):
        """rt_multi_upload_triangles from device memory of the first context's device: Tracer.upload_triangles_device's arguments.  The
        handle has no stream of the caller's, so a tensor's upload is fenced: torch's current stream is synchronised before the call and
        the device after it (the tensor may be overwritten at once)."""
        tensor = _is_tensor(tris)
        ptr, n, device = _device_triangles(tris, n)
        _arm_device_geometry(self)
        if tensor:
            import torch
            torch.cuda.current_stream(device).synchronize()
        rc = self._lib.rt_multi_upload_triangles(self._handle, c_void_p(ptr), n)
        if tensor:
            torch.cuda.synchronize(device)
        self._check(rc, "rt_multi_upload_triangles")

    def reset_accum(self):
        self._check(self._lib.rt_multi_reset_accum(self._handle), "rt_multi_reset_accum")

    def render(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_multi_render(self._handle, first_frame, n_frames), "rt_multi_render")

    def trace_rays(self, rays) -> np.ndarray:
        """rt_multi_trace_rays: Tracer.trace_rays over the contexts (host arrays), one contiguous slice of the batch each."""
        return self._query("rt_multi_trace_rays", rays)

    def occluded(self, rays) -> np.ndarray:
        """rt_multi_occluded: Tracer.occluded over the contexts (host arrays)."""
        return self._query("rt_multi_occluded", rays)

    def trace_hits(self, rays, max_hits=HITS_DEFAULT_MAX, both_sides=False, count_all=False) -> np.ndarray:
        """rt_multi_trace_hits: Tracer.trace_hits over the contexts (host arrays), one contiguous slice of the batch each."""
        return self._query("rt_multi_trace_hits", rays, _hits_params(max_hits, both_sides, count_all))

    def closest_points(self, points) -> np.ndarray:
        """rt_multi_closest_points: Tracer.closest_points over the contexts (host arrays), one contiguous slice of the batch each."""
        return self._query("rt_multi_closest_points", points)

    def trace_radiance(self, rays, samples=None, seed=0, first_index=0) -> np.ndarray:
        """rt_multi_trace_radiance: Tracer.trace_radiance over the contexts (host arrays), every ray keeping its stream index."""
        return self._query("rt_multi_trace_radiance", rays, _radiance_params(samples, seed, first_index))

    def gather(self, points, samples=None, seed=0, first_index=0, mode=GATHER_COSINE) -> np.ndarray:
        """rt_multi_gather: Tracer.gather over the contexts (host arrays), every point keeping its stream index."""
        return self._query("rt_multi_gather", points, self._gather_params(samples, seed, first_index, mode))

    def visibility(self, points, samples=None, seed=0, first_index=0, mode=VIS_COSINE) -> np.ndarray:
        """rt_multi_visibility: Tracer.visibility over the contexts (host arrays), every point keeping its stream index."""
        return self._query("rt_multi_visibility", points, _visibility_params(samples, seed, first_index, mode))

    def render_params(self, first_frame: int, params):
        """rt_multi_render_params: every context renders its bands with the per-frame uniforms params[f], then one gather."""
        p, n = _params_run(params)
        self._call("rt_multi_render_params", int(first_frame), n, _ptr(p))
        if n:
            self._shape = (int(p[0]["height"]), int(p[0]["width"]))
            self._params = p[-1].copy()

    def read_accum(self) -> np.ndarray:
        return self._plane("rt_multi_read_accum", self._image_shape() + (4,))

    # -- feature buffers
    def render_aov(self, first_frame: int, n_frames: int):
        """rt_multi_render_aov: every context accumulates the feature frames of its bands."""
        self._check(self._lib.rt_multi_render_aov(self._handle, int(first_frame), int(n_frames)), "rt_multi_render_aov")

    def read_aov(self, which: int) -> np.ndarray:
        """rt_multi_read_aov: the assembled plane, shape (H, W, 4), row 0 = bottom."""
        return self._plane("rt_multi_read_aov", self._image_shape() + (4,), int(which))

    def reset_aov(self):
        self._check(self._lib.rt_multi_reset_aov(self._handle), "rt_multi_reset_aov")

    def aov_info(self) -> list:
        """rt_get_aov_info of every context, in order"""
        out = []
        for i in range(self.count()):
            s = np.zeros((), AOV_INFO)
            rc = self._lib.rt_get_aov_info(self._lib.rt_multi_context(self._handle, i), _ptr(s))
            if rc != 0:
                raise RtError(f"rt_get_aov_info on context {i} failed ({rc})")
            out.append({k: s[k].item() for k in AOV_INFO.names})
        return out

    # -- denoiser
    def denoise(self, **params):
        """rt_multi_denoise: image and feature planes gathered to the first device, Tracer.denoise's filter there."""
        self._filter("rt_multi_denoise", _DENOISE, params)
        self._denoise_last = dict(DENOISE_DEFAULTS, **params)

    def read_denoised(self) -> np.ndarray:
        return self._plane("rt_multi_read_denoised", self._image_shape() + (4,))

    def read_denoised_display(self) -> np.ndarray:
        return self._display("rt_multi_read_denoised_display", self._image_shape())

    def denoise_info(self) -> dict:
        """the parameters of the last denoise() and the image size (the C-ABI keeps kernel times per context only)"""
        last = getattr(self, "_denoise_last", None)
        if last is None:
            return {"iterations": 0, "demodulate": 0, "width": 0, "height": 0}
        H, W = self._shape
        return {"iterations": int(last["iterations"]), "demodulate": int(last["demodulate"]), "width": W, "height": H}

    # -- temporal reprojection
    def temporal(self, **params):
        """rt_multi_temporal: image and feature planes gathered to the first device, Tracer.temporal's step there"""
        self._filter("rt_multi_temporal", _TEMPORAL, params)
        self._temporal_calls = getattr(self, "_temporal_calls", 0) + 1

    def reset_temporal(self):
        self._check(self._lib.rt_multi_reset_temporal(self._handle), "rt_multi_reset_temporal")
        self._temporal_calls = 0

    def read_temporal(self) -> np.ndarray:
        return self._plane("rt_multi_read_temporal", self._image_shape() + (4,))

    def read_temporal_history(self) -> np.ndarray:
        return self._plane("rt_multi_read_temporal_history", self._image_shape())

    def read_temporal_display(self) -> np.ndarray:
        return self._display("rt_multi_read_temporal_display", self._image_shape())

    def temporal_info(self) -> dict:
        """the calls since the history was last dropped and the image size (the C-ABI keeps kernel times per context only)"""
        H, W = self._shape
        return {"calls": getattr(self, "_temporal_calls", 0), "width": W, "height": H}

    def denoise_temporal(self, **params):
        self._filter("rt_multi_denoise_temporal", _DENOISE, params)
        self._denoise_last = dict(DENOISE_DEFAULTS, **params)

    # -- variance-guided denoiser
    def denoise_variance(self, **params):
        """rt_multi_denoise_variance: the gather of denoise() or denoise_temporal(), Tracer.denoise_variance's filter on the first device"""
        self._filter("rt_multi_denoise_variance", _VDENOISE, params)

    def read_variance(self) -> np.ndarray:
        return self._plane("rt_multi_read_variance", self._image_shape())

    def stats(self) -> dict:
        g = ctypes.c_double(0.0)
        d = self._record("rt_multi_get_stats", STATS, ctypes.byref(g))
        d["gatherMs"] = g.value
        return d

    def info(self) -> dict:
        """rt_multi_get_info: contexts, BVH builds summed over them, the last scene change's set-up time, peer access per context"""
        s = np.zeros((), MULTI_INFO)
        self._call("rt_multi_get_info", _ptr(s))
        n = int(s["numContexts"])
        return {"numContexts": n, "bvhBuilds": int(s["bvhBuilds"]), "lastSetupMs": float(s["lastSetupMs"]), "lastGatherMs": float(s["lastGatherMs"]),
                "device": s["device"][:min(n, 16)].tolist(), "peerAccess": s["peerAccess"][:min(n, 16)].tolist()}
