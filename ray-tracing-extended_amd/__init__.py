"""MI355X-native path tracer behind the Ray-Tracing-Extended scene surface.

The directory name carries a hyphen, so import it through `rtx_pkg.load()` (repo root), which registers it as the
module `rtx_amd`.  Only what the hot path needs lives here:

    csrc/      HIP kernels (gfx950), BVH builder and the C-ABI of include/rt.h  -> librt_mi355x.so
    _cabi.py   ctypes binding + buffer layouts
    capsule.py capsule overlap queries over the closest-point entries (option "closest_capsule")
    host.py    mirror of the reference's host components (RayTracingManager, RayTracedSphere, RayTracedMesh ...)
    host_cpp/  the same components + .unity loader as compiled C++ (librt_host.so); host_cpp_binding.py = ctypes window
    nearest.py K-nearest point queries over the closest-point entries (options "closest_k", "closest_all")
    overlap.py box overlap queries over the closest-point entries (option "closest_box")
    scenes.py  synthetic workloads of BASELINE.json configs
    sweep.py   sphere casts over the ray-query entries (option "sweep"), sphere-cast-all over rt_trace_hits (option "hits_sweep")
    unity_scene.py  loader for the reference's .unity scenes + compact scene interchange format
    distributed.py  row-strip decomposition + frame-end gather
"""
from . import _cabi, capsule, distributed, host, host_cpp_binding, imageio, nearest, overlap, scenes, sweep, unity_scene  # noqa: F401
from ._cabi import (AOV_INFO, RADIANCE_INFO, RADIANCE_PARAMS, GATHER_INFO, GATHER_PARAMS, GATHER_COSINE, GATHER_SH9, VISIBILITY_INFO, VISIBILITY_PARAMS, CLOSEST, CLOSEST_INFO, MULTIHIT, HITS_PARAMS, HITS_INFO, HITS_FRONT, HITS_BOTH, HITS_MAX, HITS_DEFAULT_MAX, VIS_COSINE, VIS_SH9, VIS_DISTANCE, DENOISE_DEFAULTS, DENOISE_INFO, DENOISE_PARAMS, TEMPORAL_DEFAULTS, TEMPORAL_INFO, TEMPORAL_PARAMS, VDENOISE_DEFAULTS, VDENOISE_INFO, VDENOISE_PARAMS, RT_AOV_ALBEDO, RT_AOV_COUNT, RT_AOV_NORMAL_DEPTH, HIT, LOCAL_CHUNK, MATERIAL, MESH_TRANSFORM, MULTI_INFO, MESHINFO, PARAMS, RAY, SPHERE, STATS, TRIANGLE, RT_INTERSECT_BRUTE,  # noqa: F401
                    RT_INTERSECT_FLAT_CHUNKS, MultiTracer, RtError, Tracer, load_library)
from .host import (Camera, EnvironmentSettings, Light, MaterialFlag, Mesh, MeshChunk, MeshSplitter, RayTracedMesh,  # noqa: F401
                   RayTracedSphere, RayTracingManager, RayTracingMaterial, Transform)
