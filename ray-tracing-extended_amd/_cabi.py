"""ctypes binding of include/rt.h (the C-ABI of the HIP path tracer) plus the buffer layouts as numpy dtypes.

The layouts are the reference's own GPU-buffer structs (Assets/Scripts/Data Types/RayTracingMaterial.cs:13-19,
Sphere.cs:5-7, Triangle.cs:8-14, MeshInfo.cs:5-9; strides asserted below: 64 / 80 / 72 / 96 bytes).

There is no CPU fallback: if the HIP library has not been built, or no GPU is present, this module raises.
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

# every symbol include/rt.h declares (tests check that the built library exports each one)
SYMBOLS = [
    "rt_create", "rt_destroy", "rt_last_error", "rt_set_stream", "rt_set_params", "rt_upload_spheres",
    "rt_upload_triangles", "rt_upload_meshinfo", "rt_set_rows", "rt_render_frame", "rt_render",
    "rt_render_counting", "rt_render_frame_flat", "rt_reset_accum", "rt_read_accum", "rt_read_last_frame",
    "rt_copy_accum_to_device", "rt_get_stats", "rt_abi_version", "rt_sizeof", "rt_set_option", "rt_set_bands", "rt_upload_local_meshes", "rt_set_mesh_transforms", "rt_read_world_geometry", "rt_read_display",
    "rt_read_bvh", "rt_read_bvh_order", "rt_write_accum", "rt_submit_frame", "rt_wait",
    "rt_multi_create", "rt_multi_destroy", "rt_multi_last_error", "rt_multi_count", "rt_multi_context", "rt_multi_set_params",
    "rt_multi_upload_spheres", "rt_multi_upload_triangles", "rt_multi_upload_meshinfo", "rt_multi_set_option", "rt_multi_reset_accum",
    "rt_multi_render", "rt_multi_read_accum", "rt_multi_get_stats", "rt_multi_get_info",
    "rt_multi_upload_local_meshes", "rt_multi_set_mesh_transforms", "rt_multi_read_display", "rt_multi_write_accum",
    "rt_render_params", "rt_submit_frame_params", "rt_multi_render_params",
    "rt_trace_rays", "rt_occluded", "rt_trace_rays_device", "rt_occluded_device", "rt_multi_trace_rays", "rt_multi_occluded",
    "rt_render_aov", "rt_read_aov", "rt_copy_aov_to_device", "rt_reset_aov", "rt_get_aov_info",
    "rt_multi_render_aov", "rt_multi_read_aov", "rt_multi_reset_aov",
    "rt_denoise", "rt_read_denoised", "rt_copy_denoised_to_device", "rt_read_denoised_display", "rt_get_denoise_info",
    "rt_multi_denoise", "rt_multi_read_denoised", "rt_multi_read_denoised_display",
    "rt_temporal", "rt_reset_temporal", "rt_read_temporal", "rt_read_temporal_history", "rt_copy_temporal_to_device",
    "rt_read_temporal_display", "rt_get_temporal_info", "rt_denoise_temporal",
    "rt_multi_temporal", "rt_multi_reset_temporal", "rt_multi_read_temporal", "rt_multi_read_temporal_history", "rt_multi_read_temporal_display",
    "rt_multi_denoise_temporal",
    "rt_denoise_variance", "rt_read_variance", "rt_copy_variance_to_device", "rt_get_vdenoise_info",
    "rt_multi_denoise_variance", "rt_multi_read_variance",
    "rt_trace_radiance", "rt_trace_radiance_device", "rt_get_radiance_info", "rt_multi_trace_radiance",
    "rt_gather", "rt_gather_device", "rt_get_gather_info", "rt_multi_gather",
    "rt_visibility", "rt_visibility_device", "rt_get_visibility_info", "rt_multi_visibility",
    "rt_closest_points", "rt_closest_points_device", "rt_get_closest_info", "rt_multi_closest_points",
    "rt_trace_hits", "rt_trace_hits_device", "rt_get_hits_info", "rt_multi_trace_hits",
]

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
    lib.rt_create.restype = c_void_p
    lib.rt_create.argtypes = [c_int]
    lib.rt_destroy.restype = None
    lib.rt_destroy.argtypes = [c_void_p]
    lib.rt_last_error.restype = c_char_p
    lib.rt_last_error.argtypes = [c_void_p]
    lib.rt_set_stream.argtypes = [c_void_p, c_void_p]
    lib.rt_set_params.argtypes = [c_void_p, c_void_p]
    for n in ("rt_upload_spheres", "rt_upload_triangles", "rt_upload_meshinfo"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int]
    lib.rt_set_rows.argtypes = [c_void_p, c_int, c_int]
    lib.rt_set_option.argtypes = [c_void_p, c_char_p, c_int]
    lib.rt_set_bands.argtypes = [c_void_p, c_int, c_int]
    lib.rt_upload_local_meshes.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int]
    lib.rt_set_mesh_transforms.argtypes = [c_void_p, c_void_p, c_int]
    lib.rt_read_world_geometry.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int]
    lib.rt_render_frame.argtypes = [c_void_p, c_int]
    lib.rt_render_frame_flat.argtypes = [c_void_p, c_int]
    lib.rt_render.argtypes = [c_void_p, c_int, c_int]
    lib.rt_render_counting.argtypes = [c_void_p, c_int, c_int]
    lib.rt_reset_accum.argtypes = [c_void_p]
    lib.rt_submit_frame.argtypes = [c_void_p, c_int]
    lib.rt_wait.argtypes = [c_void_p]
    lib.rt_render_params.argtypes = [c_void_p, c_int, c_int, c_void_p]
    lib.rt_submit_frame_params.argtypes = [c_void_p, c_int, c_void_p]
    lib.rt_multi_render_params.argtypes = [c_void_p, c_int, c_int, c_void_p]
    lib.rt_read_accum.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_read_last_frame.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_copy_accum_to_device.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_get_stats.argtypes = [c_void_p, c_void_p]
    lib.rt_read_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_read_bvh.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    lib.rt_read_bvh_order.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_write_accum.argtypes = [c_void_p, POINTER(c_float), c_size_t, c_int]
    lib.rt_abi_version.restype = c_int
    lib.rt_sizeof.argtypes = [c_char_p]
    lib.rt_multi_create.restype = c_void_p
    lib.rt_multi_create.argtypes = [POINTER(c_int), c_int]
    lib.rt_multi_destroy.restype = None
    lib.rt_multi_destroy.argtypes = [c_void_p]
    lib.rt_multi_last_error.restype = c_char_p
    lib.rt_multi_last_error.argtypes = [c_void_p]
    lib.rt_multi_count.argtypes = [c_void_p]
    lib.rt_multi_context.restype = c_void_p
    lib.rt_multi_context.argtypes = [c_void_p, c_int]
    lib.rt_multi_set_params.argtypes = [c_void_p, c_void_p]
    for n in ("rt_multi_upload_spheres", "rt_multi_upload_triangles", "rt_multi_upload_meshinfo"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int]
    lib.rt_multi_set_option.argtypes = [c_void_p, c_char_p, c_int]
    lib.rt_multi_reset_accum.argtypes = [c_void_p]
    lib.rt_multi_render.argtypes = [c_void_p, c_int, c_int]
    lib.rt_multi_read_accum.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_multi_get_stats.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.rt_multi_get_info.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_upload_local_meshes.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int]
    lib.rt_multi_set_mesh_transforms.argtypes = [c_void_p, c_void_p, c_int]
    lib.rt_multi_read_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_multi_write_accum.argtypes = [c_void_p, POINTER(c_float), c_size_t, c_int]
    for n in ("rt_trace_rays", "rt_occluded", "rt_trace_rays_device", "rt_occluded_device", "rt_multi_trace_rays", "rt_multi_occluded"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.rt_render_aov.argtypes = [c_void_p, c_int, c_int]
    lib.rt_read_aov.argtypes = [c_void_p, c_int, POINTER(c_float), c_size_t]
    lib.rt_copy_aov_to_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    lib.rt_reset_aov.argtypes = [c_void_p]
    lib.rt_get_aov_info.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_render_aov.argtypes = [c_void_p, c_int, c_int]
    lib.rt_multi_read_aov.argtypes = [c_void_p, c_int, POINTER(c_float), c_size_t]
    lib.rt_multi_reset_aov.argtypes = [c_void_p]
    lib.rt_denoise.argtypes = [c_void_p, c_void_p]
    lib.rt_read_denoised.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_copy_denoised_to_device.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_read_denoised_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_get_denoise_info.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_denoise.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_read_denoised.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_multi_read_denoised_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_temporal.argtypes = [c_void_p, c_void_p]
    lib.rt_reset_temporal.argtypes = [c_void_p]
    lib.rt_read_temporal.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_read_temporal_history.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_copy_temporal_to_device.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_read_temporal_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_get_temporal_info.argtypes = [c_void_p, c_void_p]
    lib.rt_denoise_temporal.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_temporal.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_reset_temporal.argtypes = [c_void_p]
    lib.rt_multi_read_temporal.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_multi_read_temporal_history.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_multi_read_temporal_display.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_multi_denoise_temporal.argtypes = [c_void_p, c_void_p]
    lib.rt_denoise_variance.argtypes = [c_void_p, c_void_p]
    lib.rt_read_variance.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    lib.rt_copy_variance_to_device.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.rt_get_vdenoise_info.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_denoise_variance.argtypes = [c_void_p, c_void_p]
    lib.rt_multi_read_variance.argtypes = [c_void_p, POINTER(c_float), c_size_t]
    for n in ("rt_trace_radiance", "rt_trace_radiance_device", "rt_multi_trace_radiance"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.rt_get_radiance_info.argtypes = [c_void_p, c_void_p]
    for n in ("rt_gather", "rt_gather_device", "rt_multi_gather"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.rt_get_gather_info.argtypes = [c_void_p, c_void_p]
    for n in ("rt_visibility", "rt_visibility_device", "rt_multi_visibility"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.rt_get_visibility_info.argtypes = [c_void_p, c_void_p]
    for n in ("rt_closest_points", "rt_closest_points_device", "rt_multi_closest_points"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.rt_get_closest_info.argtypes = [c_void_p, c_void_p]
    for n in ("rt_trace_hits", "rt_trace_hits_device", "rt_multi_trace_hits"):
        getattr(lib, n).argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.rt_get_hits_info.argtypes = [c_void_p, c_void_p]
    for n in SYMBOLS:
        f = getattr(lib, n)
        if f.restype is None or n in ("rt_create", "rt_last_error", "rt_destroy", "rt_multi_create", "rt_multi_destroy", "rt_multi_last_error",
                                      "rt_multi_context"):
            continue
        f.restype = c_int
    for name, dt in (("rt_material", MATERIAL), ("rt_sphere", SPHERE), ("rt_triangle", TRIANGLE),
                     ("rt_meshinfo", MESHINFO), ("rt_params", PARAMS), ("rt_stats", STATS),
                     ("rt_mesh_transform", MESH_TRANSFORM), ("rt_local_chunk", LOCAL_CHUNK), ("rt_multi_info", MULTI_INFO),
                     ("rt_ray", RAY), ("rt_hit", HIT), ("rt_aov_info", AOV_INFO),
                     ("rt_denoise_params", DENOISE_PARAMS), ("rt_denoise_info", DENOISE_INFO),
                     ("rt_temporal_params", TEMPORAL_PARAMS), ("rt_temporal_info", TEMPORAL_INFO),
                     ("rt_vdenoise_params", VDENOISE_PARAMS), ("rt_vdenoise_info", VDENOISE_INFO),
                     ("rt_radiance_params", RADIANCE_PARAMS), ("rt_radiance_info", RADIANCE_INFO),
                     ("rt_gather_params", GATHER_PARAMS), ("rt_gather_info", GATHER_INFO),
                     ("rt_visibility_params", VISIBILITY_PARAMS), ("rt_visibility_info", VISIBILITY_INFO),
                     ("rt_closest", CLOSEST), ("rt_closest_info", CLOSEST_INFO),
                     ("rt_hits_params", HITS_PARAMS), ("rt_multihit", MULTIHIT), ("rt_hits_info", HITS_INFO)):
        got = lib.rt_sizeof(name.encode())
        if got != dt.itemsize:
            raise RtError(f"ABI mismatch: sizeof({name}) = {got} in the library, {dt.itemsize} in the binding")
    _lib = lib
    return lib


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


def _query_host(call, handle, rays, any_hit: bool, check, what):
    r = _ray_array(rays)
    out = np.zeros(r.shape[0], np.uint8) if any_hit else np.zeros(r.shape[0], HIT)
    check(call(handle, r.ctypes.data_as(c_void_p), int(r.shape[0]), out.ctypes.data_as(c_void_p)), what)
    return out


def _hits_params(max_hits, both_sides, count_all):
    """a HITS_PARAMS record"""
    p = np.zeros((), HITS_PARAMS)
    p["maxHits"], p["mode"], p["countAll"] = int(max_hits), HITS_BOTH if both_sides else HITS_FRONT, int(bool(count_all))
    return p


def _hits_host(call, handle, rays, params, check, what):
    r = _ray_array(rays)
    K = int(params["maxHits"])
    if not 1 <= K <= HITS_MAX:
        raise RtError(f"{what}: max_hits = {K} outside 1..{HITS_MAX}")
    out = np.zeros((r.shape[0], K), MULTIHIT)
    check(call(handle, r.ctypes.data_as(c_void_p), int(r.shape[0]), params.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p)), what)
    return out


def _closest_host(call, handle, points, check, what):
    r = _ray_array(points)
    out = np.zeros(r.shape[0], CLOSEST)
    check(call(handle, r.ctypes.data_as(c_void_p), int(r.shape[0]), out.ctypes.data_as(c_void_p)), what)
    return out


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


def _radiance_shape(n, params):
    return (n, 4)


def _sampled_host(call, handle, items, params, shape, check, what):
    """A host entry of a sampled family (radiance, gather, visibility; a context's or a MultiTracer's): items as _ray_array takes them,
    params a record or None -> float32 of shape(n, params)"""
    r = _ray_array(items)
    out = np.zeros(shape(r.shape[0], params), np.float32)
    check(call(handle, r.ctypes.data_as(c_void_p), int(r.shape[0]), None if params is None else params.ctypes.data_as(c_void_p),
               out.ctypes.data_as(c_void_p)), what)
    return out


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


def _denoise_params(params: dict):
    """None (the library's defaults) when no field is given; else a DENOISE_PARAMS record: the defaults of include/rt.h with the given
    fields (iterations, demodulate, sigmaColour, sigmaNormal, sigmaDepth) replaced"""
    if not params:
        return None
    p = np.zeros((), DENOISE_PARAMS)
    for k, v in DENOISE_DEFAULTS.items():
        p[k] = v
    for k, v in params.items():
        if k not in DENOISE_DEFAULTS:
            raise TypeError(f"denoise: unknown parameter {k!r} (one of {sorted(DENOISE_DEFAULTS)})")
        p[k] = v
    return p


def _vdenoise_params(params: dict):
    """None (the library's defaults) when no field is given; else a VDENOISE_PARAMS record: the defaults of include/rt.h with the given
    fields (iterations, demodulate, source, sigmaLuminance, sigmaNormal, sigmaDepth) replaced"""
    if not params:
        return None
    p = np.zeros((), VDENOISE_PARAMS)
    for k, v in VDENOISE_DEFAULTS.items():
        p[k] = v
    for k, v in params.items():
        if k not in VDENOISE_DEFAULTS:
            raise TypeError(f"denoise_variance: unknown parameter {k!r} (one of {sorted(VDENOISE_DEFAULTS)})")
        p[k] = v
    return p


def _temporal_params(params: dict):
    """None (the library's defaults) when no field is given; else a TEMPORAL_PARAMS record: the defaults of include/rt.h with the given
    fields (maxHistory, depthTolerance, normalTolerance) replaced"""
    if not params:
        return None
    p = np.zeros((), TEMPORAL_PARAMS)
    for k, v in TEMPORAL_DEFAULTS.items():
        p[k] = v
    for k, v in params.items():
        if k not in TEMPORAL_DEFAULTS:
            raise TypeError(f"temporal: unknown parameter {k!r} (one of {sorted(TEMPORAL_DEFAULTS)})")
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


class Tracer:
    """One rt_ctx.  Thin, exception-raising wrapper; semantics are those documented in include/rt.h."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = self._lib.rt_create(device)
        if not self._ctx:
            raise RtError("rt_create failed: " + (self._lib.rt_last_error(None) or b"").decode())
        self._params = None

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.rt_destroy(self._ctx)
            self._ctx = None

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
            raise RtError(f"{what} failed ({rc}): " + (self._lib.rt_last_error(self._ctx) or b"").decode())

    # -- uploads
    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._params = p.copy()
        self._check(self._lib.rt_set_params(self._ctx, p.ctypes.data_as(c_void_p)), "rt_set_params")

    def upload(self, spheres=None, triangles=None, meshinfo=None):
        if spheres is not None:
            a, ptr, n = _as_buffer(spheres, SPHERE)
            self._check(self._lib.rt_upload_spheres(self._ctx, ptr, n), "rt_upload_spheres")
        if triangles is not None:
            a, ptr, n = _as_buffer(triangles, TRIANGLE)
            self._check(self._lib.rt_upload_triangles(self._ctx, ptr, n), "rt_upload_triangles")
        if meshinfo is not None:
            a, ptr, n = _as_buffer(meshinfo, MESHINFO)
            self._check(self._lib.rt_upload_meshinfo(self._ctx, ptr, n), "rt_upload_meshinfo")

    def upload_triangles_device(self, tris, n=None):
        """rt_upload_triangles from device memory (option "device_geometry", which this sets to 1 unless set_option has set it): a
        contiguous float32 CUDA tensor (n, 18) on the context's device — the copy is ordered with torch's current stream as trace_rays'
        device entry is, so the tensor may be overwritten on that stream right after the call — or an int device pointer and n, copied on
        the context's stream.  With the option set to 0 this raises before anything is called: a device pointer never reaches the host
        path."""
        tensor = _is_tensor(tris)
        ptr, n, device = _device_triangles(tris, n)
        _arm_device_geometry(self)
        call = lambda: self._lib.rt_upload_triangles(self._ctx, c_void_p(ptr), n)      # noqa: E731
        if tensor:
            self._on_torch_stream(device, call, "rt_upload_triangles")
        else:
            self._check(call(), "rt_upload_triangles")

    # -- on-device geometry pipeline
    def upload_local_meshes(self, local_tris, chunks, n_meshes: int):
        t, tp, nt = _as_buffer(local_tris, TRIANGLE)
        ch, cp, nc = _as_buffer(chunks, LOCAL_CHUNK)
        self._local_counts = (nt, nc)
        self._check(self._lib.rt_upload_local_meshes(self._ctx, tp, nt, cp, nc, int(n_meshes)), "rt_upload_local_meshes")

    def set_mesh_transforms(self, transforms):
        x, xp, n = _as_buffer(transforms, MESH_TRANSFORM)
        self._check(self._lib.rt_set_mesh_transforms(self._ctx, xp, n), "rt_set_mesh_transforms")

    def read_world_geometry(self):
        nt, nc = self._local_counts
        tris, infos = np.zeros(nt, TRIANGLE), np.zeros(nc, MESHINFO)
        self._check(self._lib.rt_read_world_geometry(self._ctx, tris.ctypes.data_as(c_void_p), nt,
                                                     infos.ctypes.data_as(c_void_p), nc), "rt_read_world_geometry")
        return tris, infos

    def set_rows(self, row0: int, nrows: int):
        self._rows = (row0, nrows)
        self._check(self._lib.rt_set_rows(self._ctx, row0, nrows), "rt_set_rows")

    def set_bands(self, first_band: int, band_stride: int, height: int = None):
        H = int(self._params["height"]) if height is None else height
        self._rows = (first_band * 8, sum(min(8, H - y) for y in range(first_band * 8, H, band_stride * 8)))
        self._check(self._lib.rt_set_bands(self._ctx, first_band, band_stride), "rt_set_bands")

    def set_option(self, name: str, value: int):
        self._check(self._lib.rt_set_option(self._ctx, name.encode(), int(value)), f"rt_set_option({name})")
        if name == "device_geometry":
            self._device_geometry = int(value)

    def set_stream(self, stream_ptr):
        self._check(self._lib.rt_set_stream(self._ctx, c_void_p(stream_ptr)), "rt_set_stream")
        self._stream = stream_ptr

    # -- ray queries
    def trace_rays(self, rays):
        """rt_trace_rays: the closest hit of every ray.  rays: a RAY array or float32 (n, 8) -> a HIT array.  A float32 CUDA tensor
        (n, 8) on the context's device takes the device entry instead and returns a float32 (n, 16) tensor (the HIT records)."""
        if _is_tensor(rays):
            return self._query_device(rays, False)
        return _query_host(self._lib.rt_trace_rays, self._ctx, rays, False, self._check, "rt_trace_rays")

    def occluded(self, rays):
        """rt_occluded: 1 where the closest-hit query of the ray would hit.  rays as for trace_rays -> uint8 (n,) (array or tensor)."""
        if _is_tensor(rays):
            return self._query_device(rays, True)
        return _query_host(self._lib.rt_occluded, self._ctx, rays, True, self._check, "rt_occluded")

    def _query_device(self, rays, any_hit: bool):
        """The device entries on torch tensors, ordered with torch's current stream both ways: the context runs the call on that stream
        (rt_set_stream: the stream first waits for what the context enqueued before) and goes back to its own stream (or the one set_stream
        gave it) afterwards, which then waits for the query (rt_set_stream's switch is ordered) — so torch's later work on the stream sees
        the results, and the context's next upload, geometry pass or render cannot overtake the query.  torch's legacy default stream has no handle the
        library can take (NULL means the context's own stream), so there the call is fenced: torch's stream is synchronised before it and
        the device after it.  (torch ships its own HIP runtime: import torch before the library is loaded, so that both use that one.)"""
        import torch
        rays = self._ray_tensor(rays)
        n = int(rays.shape[0])
        out = torch.empty((n,), dtype=torch.uint8, device=rays.device) if any_hit else torch.empty((n, 16), dtype=torch.float32, device=rays.device)
        call = self._lib.rt_occluded_device if any_hit else self._lib.rt_trace_rays_device
        what = "rt_occluded_device" if any_hit else "rt_trace_rays_device"
        self._on_torch_stream(rays.device, lambda: call(self._ctx, c_void_p(rays.data_ptr()), n, c_void_p(out.data_ptr())), what)
        return out

    @staticmethod
    def _ray_tensor(rays):
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays: a float32 (n, 8) tensor, not {rays.dtype} {tuple(rays.shape)}")
        return rays.contiguous()

    def _on_torch_stream(self, device, call, what):
        """call() — a device entry — ordered with torch's current stream of `device` as _query_device describes"""
        import torch
        stream = torch.cuda.current_stream(device)
        handle = int(stream.cuda_stream)
        if handle == 0:
            stream.synchronize()
            rc = call()
            torch.cuda.synchronize(device)
            self._check(rc, what)
            return
        self._check(self._lib.rt_set_stream(self._ctx, c_void_p(handle)), "rt_set_stream")
        try:
            rc = call()
        finally:
            self._lib.rt_set_stream(self._ctx, c_void_p(getattr(self, "_stream", None) or None))
        self._check(rc, what)

    def _sampled(self, name, items, params, shape):
        """A sampled family (radiance, gather, visibility): its host entry `name` on arrays, `name`_device on a float32 CUDA tensor (n, 8) of the
        context's device, ordered with torch's current stream as _query_device describes; -> float32 of shape(n, params) either way"""
        if not _is_tensor(items):
            return _sampled_host(getattr(self._lib, name), self._ctx, items, params, shape, self._check, name)
        import torch
        items = self._ray_tensor(items)
        n = int(items.shape[0])
        out = torch.empty(shape(n, params), dtype=torch.float32, device=items.device)
        qp = None if params is None else params.ctypes.data_as(c_void_p)
        call = getattr(self._lib, name + "_device")
        self._on_torch_stream(items.device, lambda: call(self._ctx, c_void_p(items.data_ptr()), n, qp, c_void_p(out.data_ptr())), name + "_device")
        return out

    # -- radiance queries
    def trace_radiance(self, rays, samples=None, seed=0, first_index=0):
        """rt_trace_radiance: Trace along every ray, averaged over `samples` runs (None: the context's numRaysPerPixel, seed 0, first
        index 0).  rays: a RAY array or float32 (n, 8) -> float32 (n, 4).  A float32 CUDA tensor (n, 8) on the context's device takes the
        device entry, ordered with torch's current stream as trace_rays is, and returns a float32 (n, 4) tensor."""
        return self._sampled("rt_trace_radiance", rays, _radiance_params(samples, seed, first_index), _radiance_shape)

    def radiance_info(self) -> dict:
        s = np.zeros((), RADIANCE_INFO)
        self._check(self._lib.rt_get_radiance_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_radiance_info")
        return {k: s[k].item() for k in RADIANCE_INFO.names if k != "_reserved"}

    # -- gather queries
    def gather(self, points, samples=None, seed=0, first_index=0, mode=GATHER_COSINE):
        """rt_gather: the light arriving at every point over `samples` directions drawn on the device (None: the context's
        numRaysPerPixel, seed 0, first index 0, mode 0).  points: a RAY array or float32 (n, 8) — origin, tMax, NORMAL, - .  mode
        GATHER_COSINE -> float32 (n, 4), the mean radiance over the cosine lobe (irradiance = pi times it); GATHER_SH9 -> float32
        (n, 9, 4), the SH coefficients of the incoming radiance.  A float32 CUDA tensor (n, 8) on the context's device takes the device
        entry, ordered with torch's current stream as trace_rays is, and returns a tensor of that shape.  samples=None with a seed, first
        index or mode (gather(points, mode=GATHER_SH9)) is the numRaysPerPixel of the params set last, as the library's own default is."""
        q = _gather_params(samples, seed, first_index, mode, None if self._params is None else int(self._params["numRaysPerPixel"]))
        return self._sampled("rt_gather", points, q, _gather_shape)

    def gather_info(self) -> dict:
        s = np.zeros((), GATHER_INFO)
        self._check(self._lib.rt_get_gather_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_gather_info")
        return {k: s[k].item() for k in GATHER_INFO.names}

    # -- visibility gathers
    def visibility(self, points, samples=None, seed=0, first_index=0, mode=VIS_COSINE):
        """rt_visibility: how open every point is over `samples` directions drawn on the device — rt_gather's directions, bit for bit
        (None: 64 samples).  points: a RAY array or float32 (n, 8) — origin, the reach tMax, NORMAL, - .  No params are needed.  mode
        VIS_COSINE -> float32 (n, 4): the bent normal (the mean open direction, not normalised) and the visibility fraction (ambient
        occlusion = 1 - it); VIS_SH9 -> float32 (n, 12): nine SH coefficients of the visibility function, the visibility fraction, 0, 0;
        VIS_DISTANCE -> float32 (n, 4): mean distance (a miss counts the reach), mean squared distance, hit fraction, 1.  A float32 CUDA
        tensor (n, 8) on the context's device takes the device entry, ordered with torch's current stream as trace_rays is, and returns a
        tensor of that shape."""
        return self._sampled("rt_visibility", points, _visibility_params(samples, seed, first_index, mode), _visibility_shape)

    visibility_device = visibility          # (a tensor takes rt_visibility_device; the name says so at the call site)

    def visibility_info(self) -> dict:
        s = np.zeros((), VISIBILITY_INFO)
        self._check(self._lib.rt_get_visibility_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_visibility_info")
        return {k: s[k].item() for k in VISIBILITY_INFO.names}

    # -- closest-point queries
    def closest_points(self, points):
        """rt_closest_points: the nearest sphere or triangle to every point, where on it, how far and on which side.  points: a RAY array
        or float32 (n, 8) — the point, the search radius in tMax (inf: unbounded), the rest unread -> a CLOSEST array.  No params are
        needed.  A float32 CUDA tensor (n, 8) on the context's device takes the device entry, ordered with torch's current stream as
        trace_rays is, and returns a float32 (n, 16) tensor (the CLOSEST records)."""
        if not _is_tensor(points):
            return _closest_host(self._lib.rt_closest_points, self._ctx, points, self._check, "rt_closest_points")
        import torch
        points = self._ray_tensor(points)
        n = int(points.shape[0])
        out = torch.empty((n, 16), dtype=torch.float32, device=points.device)
        self._on_torch_stream(points.device, lambda: self._lib.rt_closest_points_device(self._ctx, c_void_p(points.data_ptr()), n, c_void_p(out.data_ptr())),
                              "rt_closest_points_device")
        return out

    closest_points_device = closest_points  # (a tensor takes rt_closest_points_device; the name says so at the call site)

    def closest_info(self) -> dict:
        s = np.zeros((), CLOSEST_INFO)
        self._check(self._lib.rt_get_closest_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_closest_info")
        return {k: s[k].item() for k in CLOSEST_INFO.names if k != "_reserved"}

    # -- multi-hit ray queries
    def trace_hits(self, rays, max_hits=HITS_DEFAULT_MAX, both_sides=False, count_all=False):
        """rt_trace_hits: the first max_hits (1..8) surfaces along every ray, nearest first.  rays: a RAY array or float32 (n, 8) -> a
        MULTIHIT array (n, max_hits); records past a ray's last hit are empty (kind 0, dst inf).  both_sides: back faces of triangles
        and the exit points of spheres count too (side = -1).  count_all: hitCount is the number of all hits below tMax instead of
        min(hits, max_hits).  No params are needed.  A float32 CUDA tensor (n, 8) on the context's device takes the device entry,
        ordered with torch's current stream as trace_rays is, and returns a float32 (n, max_hits, 16) tensor (the MULTIHIT records)."""
        p = _hits_params(max_hits, both_sides, count_all)
        if not _is_tensor(rays):
            return _hits_host(self._lib.rt_trace_hits, self._ctx, rays, p, self._check, "rt_trace_hits")
        import torch
        rays = self._ray_tensor(rays)
        n, K = int(rays.shape[0]), int(p["maxHits"])
        if not 1 <= K <= HITS_MAX:
            raise RtError(f"rt_trace_hits_device: max_hits = {K} outside 1..{HITS_MAX}")
        out = torch.empty((n, K, 16), dtype=torch.float32, device=rays.device)
        self._on_torch_stream(rays.device, lambda: self._lib.rt_trace_hits_device(self._ctx, c_void_p(rays.data_ptr()), n, p.ctypes.data_as(c_void_p),
                                                                                  c_void_p(out.data_ptr())), "rt_trace_hits_device")
        return out

    trace_hits_device = trace_hits  # (a tensor takes rt_trace_hits_device; the name says so at the call site)

    def hits_info(self) -> dict:
        s = np.zeros((), HITS_INFO)
        self._check(self._lib.rt_get_hits_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_hits_info")
        return {k: s[k].item() for k in HITS_INFO.names}

    # -- rendering
    def render_frame(self, frame: int):
        self._check(self._lib.rt_render_frame(self._ctx, frame), "rt_render_frame")

    def render(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_render(self._ctx, first_frame, n_frames), "rt_render")

    def render_params(self, first_frame: int, params):
        """rt_render_params: frame first_frame + f with the uniforms params[f] (a PARAMS array; all entries share the settings)."""
        p, n = _params_run(params)
        self._check(self._lib.rt_render_params(self._ctx, int(first_frame), n, p.ctypes.data_as(c_void_p)), "rt_render_params")
        if n:
            self._params = p[-1].copy()

    def render_counting(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_render_counting(self._ctx, first_frame, n_frames), "rt_render_counting")

    def render_frame_flat(self, frame: int):
        self._check(self._lib.rt_render_frame_flat(self._ctx, frame), "rt_render_frame_flat")

    def reset_accum(self):
        self._check(self._lib.rt_reset_accum(self._ctx), "rt_reset_accum")

    # -- read-back
    def _strip_shape(self):
        W, H = int(self._params["width"]), int(self._params["height"])
        rows = getattr(self, "_rows", (0, H))[1]
        return rows, W

    def read_accum(self) -> np.ndarray:
        rows, W = self._strip_shape()
        out = np.empty((rows, W, 4), np.float32)
        self._check(self._lib.rt_read_accum(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_accum")
        return out

    def submit_frame(self, frame_index: int):
        """Queue one frame (returns at once); wait() or any other call makes sure it is in resultTexture."""
        self._check(self._lib.rt_submit_frame(self._ctx, int(frame_index)), "rt_submit_frame")

    def submit_frame_params(self, frame_index: int, params):
        """rt_submit_frame_params: queue one frame with its own uniforms (a camera move does not wait for the queue)."""
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._check(self._lib.rt_submit_frame_params(self._ctx, int(frame_index), p.ctypes.data_as(c_void_p)), "rt_submit_frame_params")
        self._params = p.copy()

    def wait(self):
        self._check(self._lib.rt_wait(self._ctx), "rt_wait")

    def write_accum(self, rgba, frames_rendered: int):
        """Restore a saved resultTexture (as read_accum returned it) and the frame counter."""
        a = np.ascontiguousarray(rgba, np.float32)
        self._check(self._lib.rt_write_accum(self._ctx, a.ctypes.data_as(POINTER(c_float)), a.size, int(frames_rendered)), "rt_write_accum")

    def read_last_frame(self) -> np.ndarray:
        rows, W = self._strip_shape()
        out = np.empty((rows, W, 4), np.float32)
        self._check(self._lib.rt_read_last_frame(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_last_frame")
        return out

    def read_display(self) -> np.ndarray:
        """resultTexture as sRGB RGBA8, shape (rows, W, 4) uint8, row 0 = bottom."""
        rows, W = self._strip_shape()
        out = np.empty((rows, W), np.uint32)
        self._check(self._lib.rt_read_display(self._ctx, out.ctypes.data_as(c_void_p), out.size), "rt_read_display")
        return out.view(np.uint8).reshape(rows, W, 4)

    def copy_accum_to_device(self, device_ptr: int, n_floats: int):
        self._check(self._lib.rt_copy_accum_to_device(self._ctx, c_void_p(device_ptr), n_floats), "rt_copy_accum_to_device")

    def read_bvh(self):
        """(f32 nodes [n, 32] float32 view, f16 nodes [n, 32] uint32) of the built BVH4 (see rt_read_bvh)."""
        n = self.stats()["numBvhNodes"]
        f32, f16 = np.zeros((n, 32), np.uint32), np.zeros((n, 32), np.uint32)
        self._check(self._lib.rt_read_bvh(self._ctx, f32.ctypes.data_as(c_void_p), f16.ctypes.data_as(c_void_p), n), "rt_read_bvh")
        return f32, f16

    def read_bvh_order(self):
        """BVH position -> uploaded triangle (see rt_read_bvh_order), uint32 [sum of the leaf counts of read_bvh()]."""
        refs = self.read_bvh()[0][:, 24:28].ravel()
        leaves = refs[((refs & 0x80000000) != 0) & (refs != 0xFFFFFFFF)]
        order = np.zeros(int(((leaves & 3) + 1).sum()), np.uint32)
        self._check(self._lib.rt_read_bvh_order(self._ctx, order.ctypes.data_as(c_void_p), order.size), "rt_read_bvh_order")
        return order

    # -- feature buffers
    def render_aov(self, first_frame: int, n_frames: int):
        """rt_render_aov: accumulate the feature frames first_frame .. first_frame + n_frames - 1 into the two planes."""
        self._check(self._lib.rt_render_aov(self._ctx, int(first_frame), int(n_frames)), "rt_render_aov")

    def read_aov(self, which: int) -> np.ndarray:
        """rt_read_aov: plane RT_AOV_ALBEDO (albedo.rgb, coverage) or RT_AOV_NORMAL_DEPTH (normal.xyz, depth) of this context's strip."""
        rows, W = self._strip_shape()
        out = np.empty((rows, W, 4), np.float32)
        self._check(self._lib.rt_read_aov(self._ctx, int(which), out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_aov")
        return out

    def copy_aov_to_device(self, which: int, device_ptr: int, n_floats: int):
        self._check(self._lib.rt_copy_aov_to_device(self._ctx, int(which), c_void_p(device_ptr), n_floats), "rt_copy_aov_to_device")

    def reset_aov(self):
        self._check(self._lib.rt_reset_aov(self._ctx), "rt_reset_aov")

    def aov_info(self) -> dict:
        s = np.zeros((), AOV_INFO)
        self._check(self._lib.rt_get_aov_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_aov_info")
        return {k: s[k].item() for k in AOV_INFO.names}

    # -- denoiser
    def denoise(self, **params):
        """rt_denoise: filter resultTexture, guided by the feature planes, into the denoised plane.  Keywords: iterations, demodulate,
        sigmaColour, sigmaNormal, sigmaDepth; none = the library's defaults."""
        p = _denoise_params(params)
        self._check(self._lib.rt_denoise(self._ctx, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_denoise")

    def _image_shape(self):
        return int(self._params["height"]), int(self._params["width"])

    def read_denoised(self) -> np.ndarray:
        H, W = self._image_shape()
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_read_denoised(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_denoised")
        return out

    def read_denoised_display(self) -> np.ndarray:
        """the denoised plane as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        H, W = self._image_shape()
        out = np.empty((H, W), np.uint32)
        self._check(self._lib.rt_read_denoised_display(self._ctx, out.ctypes.data_as(c_void_p), out.size), "rt_read_denoised_display")
        return out.view(np.uint8).reshape(H, W, 4)

    def copy_denoised_to_device(self, device_ptr: int, n_floats: int):
        self._check(self._lib.rt_copy_denoised_to_device(self._ctx, c_void_p(device_ptr), n_floats), "rt_copy_denoised_to_device")

    def denoise_info(self) -> dict:
        s = np.zeros((), DENOISE_INFO)
        self._check(self._lib.rt_get_denoise_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_denoise_info")
        return {k: s[k].item() for k in DENOISE_INFO.names}

    # -- temporal reprojection
    def temporal(self, **params):
        """rt_temporal: reproject the previous temporal colour into the current camera's view and blend resultTexture in.  Keywords:
        maxHistory, depthTolerance, normalTolerance; none = the library's defaults."""
        p = _temporal_params(params)
        self._check(self._lib.rt_temporal(self._ctx, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_temporal")

    def reset_temporal(self):
        self._check(self._lib.rt_reset_temporal(self._ctx), "rt_reset_temporal")

    def read_temporal(self) -> np.ndarray:
        H, W = self._image_shape()
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_read_temporal(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_temporal")
        return out

    def read_temporal_history(self) -> np.ndarray:
        """the history length N per pixel, shape (H, W)"""
        H, W = self._image_shape()
        out = np.empty((H, W), np.float32)
        self._check(self._lib.rt_read_temporal_history(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_temporal_history")
        return out

    def read_temporal_display(self) -> np.ndarray:
        """the temporal colour as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        H, W = self._image_shape()
        out = np.empty((H, W), np.uint32)
        self._check(self._lib.rt_read_temporal_display(self._ctx, out.ctypes.data_as(c_void_p), out.size), "rt_read_temporal_display")
        return out.view(np.uint8).reshape(H, W, 4)

    def copy_temporal_to_device(self, device_ptr: int, n_floats: int):
        self._check(self._lib.rt_copy_temporal_to_device(self._ctx, c_void_p(device_ptr), n_floats), "rt_copy_temporal_to_device")

    def temporal_info(self) -> dict:
        s = np.zeros((), TEMPORAL_INFO)
        self._check(self._lib.rt_get_temporal_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_temporal_info")
        return {k: s[k].item() for k in TEMPORAL_INFO.names if k != "_reserved"}

    def denoise_temporal(self, **params):
        """rt_denoise_temporal: Tracer.denoise with the temporal colour in place of resultTexture; read with read_denoised*"""
        p = _denoise_params(params)
        self._check(self._lib.rt_denoise_temporal(self._ctx, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_denoise_temporal")

    # -- variance-guided denoiser
    def denoise_variance(self, **params):
        """rt_denoise_variance: the variance-guided filter of resultTexture (source 0) or the temporal colour (source 1) into the denoised
        plane; read with read_denoised*, var_0 with read_variance.  Keywords: iterations, demodulate, source, sigmaLuminance,
        sigmaNormal, sigmaDepth; none = the library's defaults."""
        p = _vdenoise_params(params)
        self._check(self._lib.rt_denoise_variance(self._ctx, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_denoise_variance")

    def read_variance(self) -> np.ndarray:
        """var_0 of the last denoise_variance(), shape (H, W)"""
        H, W = self._image_shape()
        out = np.empty((H, W), np.float32)
        self._check(self._lib.rt_read_variance(self._ctx, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_read_variance")
        return out

    def copy_variance_to_device(self, device_ptr: int, n_floats: int):
        self._check(self._lib.rt_copy_variance_to_device(self._ctx, c_void_p(device_ptr), n_floats), "rt_copy_variance_to_device")

    def vdenoise_info(self) -> dict:
        s = np.zeros((), VDENOISE_INFO)
        self._check(self._lib.rt_get_vdenoise_info(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_vdenoise_info")
        return {k: s[k].item() for k in VDENOISE_INFO.names}

    def stats(self) -> dict:
        s = np.zeros((), STATS)
        self._check(self._lib.rt_get_stats(self._ctx, s.ctypes.data_as(c_void_p)), "rt_get_stats")
        return {k: (s[k].item() if s[k].ndim == 0 else s[k].tolist()) for k in STATS.names}


class MultiTracer:
    """One rt_multi: N contexts (one per entry of `devices`; a device may repeat), interleaved 8-row bands, one gather to the
    first device at the end of render()."""

    def __init__(self, devices):
        self._lib = load_library()
        arr = (c_int * len(devices))(*devices)
        self._m = self._lib.rt_multi_create(arr, len(devices))
        if not self._m:
            raise RtError("rt_multi_create failed: " + (self._lib.rt_multi_last_error(None) or b"").decode())
        self._shape = None

    def close(self):
        if getattr(self, "_m", None):
            self._lib.rt_multi_destroy(self._m)
            self._m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RtError(f"{what} failed ({rc}): " + (self._lib.rt_multi_last_error(self._m) or b"").decode())

    def count(self) -> int:
        return self._lib.rt_multi_count(self._m)

    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=PARAMS).reshape(())
        self._shape = (int(p["height"]), int(p["width"]))
        self._rays_per_pixel = int(p["numRaysPerPixel"])
        self._check(self._lib.rt_multi_set_params(self._m, p.ctypes.data_as(c_void_p)), "rt_multi_set_params")

    def upload(self, spheres=None, triangles=None, meshinfo=None):
        for arr, dt, fn in ((spheres, SPHERE, "rt_multi_upload_spheres"), (triangles, TRIANGLE, "rt_multi_upload_triangles"),
                            (meshinfo, MESHINFO, "rt_multi_upload_meshinfo")):
            if arr is not None:
                a, ptr, n = _as_buffer(arr, dt)
                self._check(getattr(self._lib, fn)(self._m, ptr, n), fn)

    def upload_local_meshes(self, local_tris, chunks, n_meshes: int):
        t, tp, nt = _as_buffer(local_tris, TRIANGLE)
        ch, cp, nc = _as_buffer(chunks, LOCAL_CHUNK)
        self._check(self._lib.rt_multi_upload_local_meshes(self._m, tp, nt, cp, nc, int(n_meshes)), "rt_multi_upload_local_meshes")

    def set_mesh_transforms(self, transforms):
        x, xp, n = _as_buffer(transforms, MESH_TRANSFORM)
        self._check(self._lib.rt_multi_set_mesh_transforms(self._m, xp, n), "rt_multi_set_mesh_transforms")

    def read_display(self) -> np.ndarray:
        """the assembled resultTexture as sRGB RGBA8, shape (H, W, 4) uint8, row 0 = bottom"""
        H, W = self._shape
        out = np.empty((H, W), np.uint32)
        self._check(self._lib.rt_multi_read_display(self._m, out.ctypes.data_as(c_void_p), out.size), "rt_multi_read_display")
        return out.view(np.uint8).reshape(H, W, 4)

    def write_accum(self, rgba, frames_rendered: int):
        """Restore a saved resultTexture (the whole image, as read_accum returned it) and the frame counter on every context."""
        a = np.ascontiguousarray(rgba, np.float32)
        self._check(self._lib.rt_multi_write_accum(self._m, a.ctypes.data_as(POINTER(c_float)), a.size, int(frames_rendered)), "rt_multi_write_accum")

    def set_option(self, name: str, value: int):
        self._check(self._lib.rt_multi_set_option(self._m, name.encode(), int(value)), f"rt_multi_set_option({name})")
        if name == "device_geometry":
            self._device_geometry = int(value)

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
        rc = self._lib.rt_multi_upload_triangles(self._m, c_void_p(ptr), n)
        if tensor:
            torch.cuda.synchronize(device)
        self._check(rc, "rt_multi_upload_triangles")

    def reset_accum(self):
        self._check(self._lib.rt_multi_reset_accum(self._m), "rt_multi_reset_accum")

    def render(self, first_frame: int, n_frames: int):
        self._check(self._lib.rt_multi_render(self._m, first_frame, n_frames), "rt_multi_render")

    def trace_rays(self, rays) -> np.ndarray:
        """rt_multi_trace_rays: Tracer.trace_rays over the contexts (host arrays), one contiguous slice of the batch each."""
        return _query_host(self._lib.rt_multi_trace_rays, self._m, rays, False, self._check, "rt_multi_trace_rays")

    def occluded(self, rays) -> np.ndarray:
        """rt_multi_occluded: Tracer.occluded over the contexts (host arrays)."""
        return _query_host(self._lib.rt_multi_occluded, self._m, rays, True, self._check, "rt_multi_occluded")

    def trace_hits(self, rays, max_hits=HITS_DEFAULT_MAX, both_sides=False, count_all=False) -> np.ndarray:
        """rt_multi_trace_hits: Tracer.trace_hits over the contexts (host arrays), one contiguous slice of the batch each."""
        return _hits_host(self._lib.rt_multi_trace_hits, self._m, rays, _hits_params(max_hits, both_sides, count_all), self._check, "rt_multi_trace_hits")

    def closest_points(self, points) -> np.ndarray:
        """rt_multi_closest_points: Tracer.closest_points over the contexts (host arrays), one contiguous slice of the batch each."""
        return _closest_host(self._lib.rt_multi_closest_points, self._m, points, self._check, "rt_multi_closest_points")

    def trace_radiance(self, rays, samples=None, seed=0, first_index=0) -> np.ndarray:
        """rt_multi_trace_radiance: Tracer.trace_radiance over the contexts (host arrays), every ray keeping its stream index."""
        return _sampled_host(self._lib.rt_multi_trace_radiance, self._m, rays, _radiance_params(samples, seed, first_index), _radiance_shape,
                             self._check, "rt_multi_trace_radiance")

    def gather(self, points, samples=None, seed=0, first_index=0, mode=GATHER_COSINE) -> np.ndarray:
        """rt_multi_gather: Tracer.gather over the contexts (host arrays), every point keeping its stream index."""
        q = _gather_params(samples, seed, first_index, mode, getattr(self, "_rays_per_pixel", None))
        return _sampled_host(self._lib.rt_multi_gather, self._m, points, q, _gather_shape, self._check, "rt_multi_gather")

    def visibility(self, points, samples=None, seed=0, first_index=0, mode=VIS_COSINE) -> np.ndarray:
        """rt_multi_visibility: Tracer.visibility over the contexts (host arrays), every point keeping its stream index."""
        return _sampled_host(self._lib.rt_multi_visibility, self._m, points, _visibility_params(samples, seed, first_index, mode), _visibility_shape,
                             self._check, "rt_multi_visibility")

    def render_params(self, first_frame: int, params):
        """rt_multi_render_params: every context renders its bands with the per-frame uniforms params[f], then one gather."""
        p, n = _params_run(params)
        self._check(self._lib.rt_multi_render_params(self._m, int(first_frame), n, p.ctypes.data_as(c_void_p)), "rt_multi_render_params")
        if n:
            self._shape = (int(p[0]["height"]), int(p[0]["width"]))
            self._rays_per_pixel = int(p[-1]["numRaysPerPixel"])

    def read_accum(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_multi_read_accum(self._m, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_accum")
        return out

    # -- feature buffers
    def render_aov(self, first_frame: int, n_frames: int):
        """rt_multi_render_aov: every context accumulates the feature frames of its bands."""
        self._check(self._lib.rt_multi_render_aov(self._m, int(first_frame), int(n_frames)), "rt_multi_render_aov")

    def read_aov(self, which: int) -> np.ndarray:
        """rt_multi_read_aov: the assembled plane, shape (H, W, 4), row 0 = bottom."""
        H, W = self._shape
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_multi_read_aov(self._m, int(which), out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_aov")
        return out

    def reset_aov(self):
        self._check(self._lib.rt_multi_reset_aov(self._m), "rt_multi_reset_aov")

    def aov_info(self) -> list:
        """rt_get_aov_info of every context, in order"""
        out = []
        for i in range(self.count()):
            s = np.zeros((), AOV_INFO)
            rc = self._lib.rt_get_aov_info(self._lib.rt_multi_context(self._m, i), s.ctypes.data_as(c_void_p))
            if rc != 0:
                raise RtError(f"rt_get_aov_info on context {i} failed ({rc})")
            out.append({k: s[k].item() for k in AOV_INFO.names})
        return out

    # -- denoiser
    def denoise(self, **params):
        """rt_multi_denoise: image and feature planes gathered to the first device, Tracer.denoise's filter there."""
        p = _denoise_params(params)
        self._check(self._lib.rt_multi_denoise(self._m, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_multi_denoise")
        self._denoise_last = dict(DENOISE_DEFAULTS, **params)

    def read_denoised(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_multi_read_denoised(self._m, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_denoised")
        return out

    def read_denoised_display(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W), np.uint32)
        self._check(self._lib.rt_multi_read_denoised_display(self._m, out.ctypes.data_as(c_void_p), out.size), "rt_multi_read_denoised_display")
        return out.view(np.uint8).reshape(H, W, 4)

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
        p = _temporal_params(params)
        self._check(self._lib.rt_multi_temporal(self._m, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_multi_temporal")
        self._temporal_calls = getattr(self, "_temporal_calls", 0) + 1

    def reset_temporal(self):
        self._check(self._lib.rt_multi_reset_temporal(self._m), "rt_multi_reset_temporal")
        self._temporal_calls = 0

    def read_temporal(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W, 4), np.float32)
        self._check(self._lib.rt_multi_read_temporal(self._m, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_temporal")
        return out

    def read_temporal_history(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W), np.float32)
        self._check(self._lib.rt_multi_read_temporal_history(self._m, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_temporal_history")
        return out

    def read_temporal_display(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W), np.uint32)
        self._check(self._lib.rt_multi_read_temporal_display(self._m, out.ctypes.data_as(c_void_p), out.size), "rt_multi_read_temporal_display")
        return out.view(np.uint8).reshape(H, W, 4)

    def temporal_info(self) -> dict:
        """the calls since the history was last dropped and the image size (the C-ABI keeps kernel times per context only)"""
        H, W = self._shape
        return {"calls": getattr(self, "_temporal_calls", 0), "width": W, "height": H}

    def denoise_temporal(self, **params):
        p = _denoise_params(params)
        self._check(self._lib.rt_multi_denoise_temporal(self._m, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_multi_denoise_temporal")
        self._denoise_last = dict(DENOISE_DEFAULTS, **params)

    # -- variance-guided denoiser
    def denoise_variance(self, **params):
        """rt_multi_denoise_variance: the gather of denoise() or denoise_temporal(), Tracer.denoise_variance's filter on the first device"""
        p = _vdenoise_params(params)
        self._check(self._lib.rt_multi_denoise_variance(self._m, p.ctypes.data_as(c_void_p) if p is not None else None), "rt_multi_denoise_variance")

    def read_variance(self) -> np.ndarray:
        H, W = self._shape
        out = np.empty((H, W), np.float32)
        self._check(self._lib.rt_multi_read_variance(self._m, out.ctypes.data_as(POINTER(c_float)), out.size), "rt_multi_read_variance")
        return out

    def stats(self) -> dict:
        s = np.zeros((), STATS)
        g = ctypes.c_double(0.0)
        self._check(self._lib.rt_multi_get_stats(self._m, s.ctypes.data_as(c_void_p), ctypes.byref(g)), "rt_multi_get_stats")
        d = {k: (s[k].item() if s[k].ndim == 0 else s[k].tolist()) for k in STATS.names}
        d["gatherMs"] = g.value
        return d

    def info(self) -> dict:
        """rt_multi_get_info: contexts, BVH builds summed over them, the last scene change's set-up time, peer access per context"""
        s = np.zeros((), MULTI_INFO)
        self._check(self._lib.rt_multi_get_info(self._m, s.ctypes.data_as(c_void_p)), "rt_multi_get_info")
        n = int(s["numContexts"])
        return {"numContexts": n, "bvhBuilds": int(s["bvhBuilds"]), "lastSetupMs": float(s["lastSetupMs"]), "lastGatherMs": float(s["lastGatherMs"]),
                "device": s["device"][:min(n, 16)].tolist(), "peerAccess": s["peerAccess"][:min(n, 16)].tolist()}
