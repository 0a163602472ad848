"""Host-side mirror of the reference's scene-description surface, above the C-ABI.

Same names, field meaning and error behaviour as the reference's C# components, so that a scene described for
the reference describes the same scene here:

    RayTracingMaterial   Assets/Scripts/Data Types/RayTracingMaterial.cs:4-29
    EnvironmentSettings  Assets/Scripts/Data Types/EnvironmentSettings.cs:4-11
    MeshChunk            Assets/Scripts/Data Types/MeshChunk.cs:6-17
    RayTracedSphere      Assets/Scripts/Render Types/RayTracedSphere.cs:5-7
    RayTracedMesh        Assets/Scripts/Render Types/RayTracedMesh.cs:17-99   (GetSubMeshes, GetMaterial)
    RayTracingManager    Assets/Scripts/RayTracingManager.cs:11-203           (settings, CreateSpheres, CreateMeshes,
                                                                                UpdateCameraParams, SetShaderParams,
                                                                                OnRenderImage, OnValidate)

All marshal arithmetic is float32 (numpy scalars), in the operation order of the C# / UnityEngine expressions it
restates (UnityEngine itself is closed source: Quaternion*Vector3, Matrix4x4.TRS and the sRGB->linear conversion of
Material.SetColor follow Unity's published formulas — "unpinned").
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from ._cabi import (LOCAL_CHUNK, MATERIAL, MESH_TRANSFORM, MESHINFO, PARAMS, RAY, RT_HIT_SPHERE, RT_HIT_TRIANGLE, SPHERE, TRIANGLE,
                    RT_INTERSECT_FLAT_CHUNKS)

f32 = np.float32


# ---- UnityEngine value types (float32) ----------------------------------------------------------------------
def _v3(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).reshape(3)


def quat_rotate(q: Sequence[float], p: np.ndarray) -> np.ndarray:
    """UnityEngine `Quaternion * Vector3` (q = x,y,z,w); p may be (3,) or (N,3).  float32 throughout."""
    x, y, z, w = (f32(c) for c in q)
    p = np.asarray(p, dtype=np.float32)
    two = f32(2)
    x2, y2, z2 = x * two, y * two, z * two
    xx, yy, zz = x * x2, y * y2, z * z2
    xy, xz, yz = x * y2, x * z2, y * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = f32(1)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    rx = (one - (yy + zz)) * px + (xy - wz) * py + (xz + wy) * pz
    ry = (xy + wz) * px + (one - (xx + zz)) * py + (yz - wx) * pz
    rz = (xz - wy) * px + (yz + wx) * py + (one - (xx + yy)) * pz
    return np.stack([rx, ry, rz], axis=-1).astype(np.float32)


def _running_extreme(v: np.ndarray, before) -> np.float32:
    """What `r = v[0]; for x in v: r = r if before(r, x) else x` leaves in r (before: np.less for Vector3.Min, np.greater for
    Vector3.Max — Mathf.Min(a, b) is a < b ? a : b and Mathf.Max a > b ? a : b), without the loop.  A NaN replaces the
    running value and the next coordinate replaces the NaN, so only what follows the last NaN counts; among equal extremes (+0 and -0)
    the last one stays."""
    v = np.asarray(v, np.float32)
    nan = np.flatnonzero(np.isnan(v))
    if len(nan):
        if nan[-1] == len(v) - 1:
            return f32(np.nan)
        v = v[nan[-1] + 1:]
    m = v.min() if before is np.less else v.max()
    return v[np.flatnonzero(v == m)[-1]]


def quat_mul(a: Sequence[float], b: Sequence[float]) -> np.ndarray:
    ax, ay, az, aw = (f32(c) for c in a)
    bx, by, bz, bw = (f32(c) for c in b)
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.float32)


@dataclass
class Transform:
    """World-space pose as the reference reads it: transform.position / rotation / lossyScale / localScale."""
    position: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    rotation: np.ndarray = field(default_factory=lambda: np.array([0, 0, 0, 1], np.float32))   # x, y, z, w
    lossyScale: np.ndarray = field(default_factory=lambda: np.ones(3, np.float32))
    localScale: Optional[np.ndarray] = None

    def __post_init__(self):
        self.position = _v3(self.position)
        self.rotation = np.asarray(self.rotation, np.float32).reshape(4)
        self.lossyScale = _v3(self.lossyScale)
        self.localScale = self.lossyScale.copy() if self.localScale is None else _v3(self.localScale)

    @property
    def localToWorldMatrix(self) -> np.ndarray:
        """Matrix4x4.TRS(position, rotation, lossyScale), row-major 4x4 float32."""
        x, y, z, w = (f32(c) for c in self.rotation)
        two, one = f32(2), f32(1)
        r = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                      [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                      [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=np.float32)
        m = np.zeros((4, 4), np.float32)
        m[:3, :3] = r * self.lossyScale[None, :]
        m[:3, 3] = self.position
        m[3, 3] = 1
        return m


# ---- data types ---------------------------------------------------------------------------------------------------
class MaterialFlag:
    NONE = 0
    CheckerPattern = 1
    InvisibleLight = 2


@dataclass
class RayTracingMaterial:
    colour: Sequence[float] = (1, 1, 1, 1)
    emissionColour: Sequence[float] = (1, 1, 1, 1)
    specularColour: Sequence[float] = (1, 1, 1, 1)
    emissionStrength: float = 0.0
    smoothness: float = 0.0
    specularProbability: float = 1.0
    flag: int = MaterialFlag.NONE

    def SetDefaultValues(self):                      # RayTracingMaterial.cs:21-28
        self.colour = (1, 1, 1, 1); self.emissionColour = (1, 1, 1, 1); self.emissionStrength = 0.0
        self.specularColour = (1, 1, 1, 1); self.smoothness = 0.0; self.specularProbability = 1.0

    def pack(self) -> np.ndarray:
        m = np.zeros((), MATERIAL)
        for k in ("colour", "emissionColour", "specularColour"):
            c = list(getattr(self, k))
            m[k] = (c + [1.0])[:4] if len(c) == 3 else c
        m["emissionStrength"] = self.emissionStrength
        m["smoothness"] = self.smoothness
        m["specularProbability"] = self.specularProbability
        m["flag"] = int(self.flag)
        return m


@dataclass
class EnvironmentSettings:
    enabled: bool = False
    groundColour: Sequence[float] = (0, 0, 0, 0)
    skyColourHorizon: Sequence[float] = (0, 0, 0, 0)
    skyColourZenith: Sequence[float] = (0, 0, 0, 0)
    sunFocus: float = 1.0
    sunIntensity: float = 0.0


@dataclass
class Bounds:
    center: np.ndarray
    size: np.ndarray

    @property
    def min(self):
        return (self.center - self.size * f32(0.5)).astype(np.float32)

    @property
    def max(self):
        return (self.center + self.size * f32(0.5)).astype(np.float32)


@dataclass
class MeshChunk:
    triangles: np.ndarray            # TRIANGLE[n]
    bounds: Bounds
    subMeshIndex: int = 0


@dataclass
class Camera:
    transform: Transform
    fieldOfView: float = 60.0
    aspect: float = 16.0 / 9.0


@dataclass
class Light:
    """Directional light: _WorldSpaceLightPos0.xyz = -forward."""
    rotation: Sequence[float] = (0, 0, 0, 1)

    @property
    def worldSpaceLightPos0(self) -> np.ndarray:
        fwd = quat_rotate(self.rotation, np.array([0, 0, 1], np.float32))
        return (-fwd).astype(np.float32)


# ---- components ---------------------------------------------------------------------------------------------------
@dataclass
class RayTracedSphere:
    transform: Transform
    material: RayTracingMaterial = field(default_factory=RayTracingMaterial)


class Mesh:
    """What MeshSplitter reads of a UnityEngine.Mesh (MeshSplitter.cs:15-23): vertices, normals, the index buffer
    (`triangles`) and the sub-mesh ranges [(indexStart, indexCount)]."""

    def __init__(self, vertices, normals, triangles, subMeshes=None):
        self.vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
        self.normals = np.asarray(normals, np.float32).reshape(-1, 3)
        self.triangles = np.asarray(triangles, np.int32).reshape(-1)
        self.subMeshes = [(0, len(self.triangles))] if subMeshes is None else [(int(a), int(b)) for a, b in subMeshes]


class RayTracedMesh:
    def __init__(self, transform: Transform, materials: List[RayTracingMaterial], localChunks: Optional[List[MeshChunk]] = None,
                 triangleCount: Optional[int] = None, enforceTriangleLimit: bool = True, sharedMesh: Optional[Mesh] = None):
        self.transform = transform
        self.materials = materials
        self.localChunks = localChunks              # [SerializeField]: the scenes carry them; None = not split yet
        self.mesh: Optional[Mesh] = None            # [SerializeField] Mesh mesh: what the cached chunks were made from
        self.sharedMesh = sharedMesh                # meshFilter.sharedMesh (None: no MeshFilter — only serialised chunks)
        if triangleCount is None:
            triangleCount = sum(len(c.triangles) for c in localChunks) if localChunks else (len(sharedMesh.triangles) // 3 if sharedMesh else 0)
        self.triangleCount = triangleCount
        self.enforceTriangleLimit = enforceTriangleLimit
        self.worldChunks: Optional[List[MeshChunk]] = None

    def GetSubMeshes(self) -> List[MeshChunk]:
        """RayTracedMesh.cs:17-54 — chunks in world space (every triangle re-transformed on the host)."""
        meshTriangles = len(self.mesh.triangles) // 3 if self.mesh is not None else self.triangleCount      # :19
        if self.enforceTriangleLimit and meshTriangles > RayTracingManager.TriangleLimit:
            raise Exception(f"Please use a mesh with fewer than {RayTracingManager.TriangleLimit} triangles")
        # Split mesh into chunks (if result is not already cached)  :24-29
        if self.sharedMesh is not None and (self.mesh is not self.sharedMesh or not self.localChunks):
            self.mesh = self.sharedMesh
            self.localChunks = MeshSplitter.CreateChunks(self.mesh)
            self.triangleCount = len(self.mesh.triangles) // 3
        pos, rot, scale = self.transform.position, self.transform.rotation, self.transform.lossyScale
        self.worldChunks = [self._UpdateWorldChunkFromLocal(c, pos, rot, scale) for c in self.localChunks]
        return self.worldChunks

    @staticmethod
    def _UpdateWorldChunkFromLocal(local: MeshChunk, pos, rot, scale) -> MeshChunk:
        """RayTracedMesh.cs:56-84 — rot * Scale(p, scale) + pos; normals rotated only; tight world AABB."""
        lt = local.triangles
        wt = np.zeros(len(lt), TRIANGLE)
        pts = []
        for k in ("posA", "posB", "posC"):
            w = (quat_rotate(rot, lt[k] * scale[None, :]) + pos[None, :]).astype(np.float32)     # PointLocalToWorld :86-89
            wt[k] = w
            pts.append(w)
        for k in ("normalA", "normalB", "normalC"):
            wt[k] = quat_rotate(rot, lt[k])                                                      # DirectionLocalToWorld :91-94
        allp = np.stack(pts, axis=1).reshape(-1, 3)                                              # A, B, C per triangle in buffer order :74-79
        bmin = np.array([_running_extreme(allp[:, a], np.less) for a in range(3)], np.float32)
        bmax = np.array([_running_extreme(allp[:, a], np.greater) for a in range(3)], np.float32)
        bounds = Bounds(((bmin + bmax) / f32(2)).astype(np.float32), (bmax - bmin).astype(np.float32))   # :82
        return MeshChunk(wt, bounds, local.subMeshIndex)

    def GetMaterial(self, subMeshIndex: int) -> RayTracingMaterial:                                  # :96-99
        return self.materials[min(subMeshIndex, len(self.materials) - 1)]


def gamma_to_linear(c: float) -> float:
    """sRGB -> linear as Unity applies in Material.SetColor when the project is in Linear colour space."""
    c = float(c)
    if c <= 0.04045:
        return c / 12.92
    if c < 1.0:
        return ((c + 0.055) / 1.055) ** 2.4
    return c ** 2.2


class RayTracingManager:
    """Frame driver / marshaller — RayTracingManager.cs.  `backend` is a Tracer (the HIP C-ABI context)."""
    TriangleLimit = 1500                                                      # RayTracingManager.cs:9

    def __init__(self, camera: Camera, light: Optional[Light] = None, width: int = 1920, height: int = 1080,
                 backend=None, linearColourSpace: bool = True):
        # settings, defaults of RayTracingManager.cs:12-17
        self.maxBounceCount = 4
        self.numRaysPerPixel = 2
        self.defocusStrength = 0.0
        self.divergeStrength = 0.3
        self.focusDistance = 1.0
        self.environmentSettings = EnvironmentSettings()
        # info
        self.numRenderedFrames = 0
        self.numMeshChunks = 0
        self.numTriangles = 0
        # scene
        self.camera = camera
        self.light = light or Light()
        self.width, self.height = int(width), int(height)
        self.spheres: List[RayTracedSphere] = []
        self.meshes: List[RayTracedMesh] = []
        self.linearColourSpace = linearColourSpace        # ProjectSettings.asset:50 (m_ActiveColorSpace: 1)
        self.intersectMode = RT_INTERSECT_FLAT_CHUNKS
        self.backend = backend
        self.deviceGeometry = False                       # True: transform / bounds / BVH refit on the GPU (rt_upload_local_meshes)
        self.deviceTriangles = None                       # a float32 (n, 18) CUDA tensor of world-space triangles, or a callable that returns
                                                          # this frame's: the caller deforms on the device, no CPU transform (InitFrame)
        self._dirty = True

    # -- RayTracingManager.cs:196-203
    def OnValidate(self):
        self.maxBounceCount = max(0, self.maxBounceCount)
        self.numRaysPerPixel = max(1, self.numRaysPerPixel)
        self.environmentSettings.sunFocus = max(1, self.environmentSettings.sunFocus)
        self.environmentSettings.sunIntensity = max(0, self.environmentSettings.sunIntensity)

    # -- RayTracingManager.cs:126-133
    def UpdateCameraParams(self, params: np.ndarray):
        deg2rad = f32(0.017453292)
        half = f32(self.camera.fieldOfView) * f32(0.5) * deg2rad
        planeHeight = f32(self.focusDistance) * f32(math.tan(float(half))) * f32(2)
        planeWidth = planeHeight * f32(self.camera.aspect)
        params["viewParams"] = (planeWidth, planeHeight, f32(self.focusDistance))
        params["camLocalToWorld"] = self.camera.transform.localToWorldMatrix.reshape(16)
        params["worldSpaceCameraPos"] = self.camera.transform.position
        params["worldSpaceLightPos0"] = self.light.worldSpaceLightPos0

    # -- RayTracingManager.cs:111-124
    def SetShaderParams(self, params: np.ndarray):
        params["maxBounceCount"] = self.maxBounceCount
        params["numRaysPerPixel"] = self.numRaysPerPixel
        params["defocusStrength"] = self.defocusStrength
        params["divergeStrength"] = self.divergeStrength
        env = self.environmentSettings
        params["environmentEnabled"] = 1 if env.enabled else 0
        for key, col in (("groundColour", env.groundColour), ("skyColourHorizon", env.skyColourHorizon),
                         ("skyColourZenith", env.skyColourZenith)):
            c = list(col) + [1.0] * (4 - len(col))
            if self.linearColourSpace:                       # Material.SetColor converts sRGB -> linear (alpha untouched)
                c = [gamma_to_linear(c[0]), gamma_to_linear(c[1]), gamma_to_linear(c[2]), c[3]]
            params[key] = c
        params["sunFocus"] = env.sunFocus
        params["sunIntensity"] = env.sunIntensity

    # -- RayTracingManager.cs:167-187
    def CreateSpheres(self) -> np.ndarray:
        out = np.zeros(len(self.spheres), SPHERE)
        for i, s in enumerate(self.spheres):
            out[i]["position"] = s.transform.position
            out[i]["radius"] = f32(s.transform.localScale[0]) * f32(0.5)
            out[i]["material"] = s.material.pack()
        return out

    # -- RayTracingManager.cs:135-164
    def CreateMeshes(self):
        tris, infos = [], []
        count = 0
        self._chunkMesh = []                                                      # chunk -> index in self.meshes (Raycast)
        for mesh_index, mesh in enumerate(self.meshes):
            for chunk in mesh.GetSubMeshes():
                self._chunkMesh.append(mesh_index)
                mi = np.zeros((), MESHINFO)
                mi["firstTriangleIndex"] = count
                mi["numTriangles"] = len(chunk.triangles)
                mi["material"] = mesh.GetMaterial(chunk.subMeshIndex).pack()
                mi["boundsMin"] = chunk.bounds.min                                # MeshInfo.cs:16-17
                mi["boundsMax"] = chunk.bounds.max
                infos.append(mi)
                tris.append(chunk.triangles)
                count += len(chunk.triangles)
        self.numMeshChunks = len(infos)
        self.numTriangles = count
        all_tris = np.concatenate(tris) if tris else np.zeros(0, TRIANGLE)
        all_info = np.array(infos, dtype=MESHINFO) if infos else np.zeros(0, MESHINFO)
        return all_tris, all_info

    # -- the same scene for the on-device geometry pipeline: local chunks once, one transform per mesh per frame
    def build_local_buffers(self):
        tris, chunks = [], []
        count = 0
        for mi, mesh in enumerate(self.meshes):
            if mesh.enforceTriangleLimit and mesh.triangleCount > RayTracingManager.TriangleLimit:
                raise Exception(f"Please use a mesh with fewer than {RayTracingManager.TriangleLimit} triangles")
            for chunk in mesh.localChunks:
                c = np.zeros((), LOCAL_CHUNK)
                c["firstTriangleIndex"], c["numTriangles"], c["meshIndex"] = count, len(chunk.triangles), mi
                c["material"] = mesh.GetMaterial(chunk.subMeshIndex).pack()
                chunks.append(c)
                tris.append(chunk.triangles)
                count += len(chunk.triangles)
        self.numMeshChunks, self.numTriangles = len(chunks), count
        return (np.concatenate(tris) if tris else np.zeros(0, TRIANGLE),
                np.array(chunks, dtype=LOCAL_CHUNK) if chunks else np.zeros(0, LOCAL_CHUNK))

    def build_transforms(self) -> np.ndarray:
        xf = np.zeros(len(self.meshes), MESH_TRANSFORM)
        for i, mesh in enumerate(self.meshes):
            xf[i]["position"], xf[i]["rotation"], xf[i]["lossyScale"] = mesh.transform.position, mesh.transform.rotation, mesh.transform.lossyScale
        return xf

    def build_buffers(self):
        """InitFrame (RayTracingManager.cs:95-109) without the device: params + the three structured buffers."""
        params = np.zeros((), PARAMS)
        params["width"], params["height"] = self.width, self.height
        params["intersectMode"] = self.intersectMode
        self.UpdateCameraParams(params)
        spheres = self.CreateSpheres()
        tris, infos = self.CreateMeshes()
        self.SetShaderParams(params)
        return params, spheres, tris, infos

    def InitFrame(self):
        if self.backend is None:
            raise RuntimeError("RayTracingManager has no backend (HIP Tracer); there is no CPU path")
        if self.deviceTriangles is not None:
            # the caller holds the world-space triangles on the device (skinning, cloth, a simulation): the chunks' ranges, materials and
            # boxes go up once — the boxes are the first pose's, so a caller whose mesh leaves them sets intersectMode to
            # RT_INTERSECT_BRUTE or uploads new ones — and every frame hands over the tensor (Tracer.upload_triangles_device: updated in
            # place while the count stays)
            params = np.zeros((), PARAMS)
            params["width"], params["height"] = self.width, self.height
            params["intersectMode"] = self.intersectMode
            self.UpdateCameraParams(params)
            self.SetShaderParams(params)
            self.backend.set_params(params)
            if self._dirty:
                self.backend.upload(spheres=self.CreateSpheres(), meshinfo=self.CreateMeshes()[1])
                self._dirty = False
            tris = self.deviceTriangles() if callable(self.deviceTriangles) else self.deviceTriangles
            self.backend.upload_triangles_device(tris)
            return
        if self.deviceGeometry:
            params = np.zeros((), PARAMS)
            params["width"], params["height"] = self.width, self.height
            params["intersectMode"] = self.intersectMode
            self.UpdateCameraParams(params)
            self.SetShaderParams(params)
            self.backend.set_params(params)
            if self._dirty:                                  # geometry: once
                self.backend.upload(spheres=self.CreateSpheres())
                self.backend.upload_local_meshes(*self.build_local_buffers(), len(self.meshes))
                self._dirty = False
            self.backend.set_mesh_transforms(self.build_transforms())    # poses: every frame (40 B per mesh)
            return
        params, spheres, tris, infos = self.build_buffers()
        self.backend.set_params(params)
        if self._dirty:
            self.backend.upload(spheres=spheres, triangles=tris, meshinfo=infos)
            self._dirty = False

    def Raycast(self, origin, direction, maxDistance: float = math.inf):
        """The picking call: what the ray origin + t * direction (t < maxDistance, in units of |direction|) hits in the scene the next frame
        traces — CalculateRayCollision (RayTracing.shader:256-297) through rt_trace_rays.  Returns (hit, component): the HIT record and the
        RayTracedSphere or RayTracedMesh it belongs to, or None on a miss."""
        self.InitFrame()                                     # the scene as OnRenderImage would trace it (uploads, mesh poses)
        ray = np.zeros(1, RAY)
        ray["origin"], ray["direction"], ray["tMax"] = _v3(origin), _v3(direction), f32(maxDistance)
        hit = self.backend.trace_rays(ray)[0]
        if hit["kind"] == RT_HIT_SPHERE:
            return hit, self.spheres[int(hit["primitive"])]
        if hit["kind"] == RT_HIT_TRIANGLE:
            mesh = int(hit["mesh"]) if self.deviceGeometry else self._chunkMesh[int(hit["chunk"])]
            return hit, self.meshes[mesh]
        return hit, None

    def RaycastAll(self, origin, direction, maxDistance: float = math.inf, maxHits: int = 8, bothSides: bool = False):
        """Physics.RaycastAll for the traced scene: everything the ray origin + t * direction (t < maxDistance) passes through in the
        scene the next frame traces, nearest first, at most maxHits (1..8) surfaces — rt_trace_hits.  bothSides: the back faces of
        triangles and the exit points of spheres count too (side = -1).  Returns the non-empty MULTIHIT records in order; hitCount ==
        maxHits in them means there may be more."""
        self.InitFrame()
        ray = np.zeros(1, RAY)
        ray["origin"], ray["direction"], ray["tMax"] = _v3(origin), _v3(direction), f32(maxDistance)
        hits = self.backend.trace_hits(ray, maxHits, bothSides)[0]
        return hits[hits["kind"] != 0]

    def TraceRadiance(self, rays, samples: int = None, seed: int = 0, firstIndex: int = 0):
        """Beyond the reference: how much light arrives along each ray in the scene the next frame traces — Trace (RayTracing.shader:300-352)
        through rt_trace_radiance, averaged over `samples` runs (None: numRaysPerPixel): light probes, lightmap texels, a camera the
        reference does not have.  rays: a RAY array or float32 (n, 8) -> float32 (n, 4), (r, g, b, 1)."""
        self.InitFrame()
        return self.backend.trace_radiance(rays, samples, seed, firstIndex)

    def TraceRadianceTensor(self, rays, samples: int = None, seed: int = 0, firstIndex: int = 0):
        """TraceRadiance for a float32 (n, 8) tensor on the tracer's device (rt_trace_radiance_device): the rays never leave the GPU and
        the result, a float32 (n, 4) tensor, is ordered with torch's current stream."""
        if not hasattr(rays, "data_ptr"):
            raise TypeError("TraceRadianceTensor: rays must be a torch tensor on the tracer's device (host arrays: TraceRadiance)")
        self.InitFrame()
        return self.backend.trace_radiance(rays, samples, seed, firstIndex)

    def Gather(self, points, samples: int = None, seed: int = 0, firstIndex: int = 0, mode: int = 0):
        """Beyond the reference: the light that arrives at each point of the scene the next frame traces, over `samples` directions the
        device draws (rt_gather; None: numRaysPerPixel).  points: a RAY array or float32 (n, 8) with the NORMAL in the direction field
        (a point on a surface is moved off it by the caller).  mode 0 -> float32 (n, 4): the mean radiance over the cosine lobe about the
        normal (irradiance = pi times it) — a lightmap texel; mode 1 -> float32 (n, 9, 4): nine SH coefficients — a light probe.  A
        tensor on the tracer's device takes rt_gather_device and returns a tensor."""
        self.InitFrame()
        return self.backend.gather(points, samples, seed, firstIndex, mode)

    def Visibility(self, points, samples: int = None, seed: int = 0, firstIndex: int = 0, mode: int = 0):
        """Beyond the reference: how open each point of the scene the next frame traces is, over `samples` directions the device draws —
        the directions Gather draws for the same seed and index (rt_visibility; None: 64).  points as for Gather, tMax the reach.  mode 0
        -> float32 (n, 4): bent normal and visibility fraction (ambient occlusion = 1 - it) — a lightmap texel; mode 1 -> float32
        (n, 12): nine SH coefficients of the visibility, the fraction, 0, 0 — a probe's sky visibility; mode 2 -> float32 (n, 4): mean
        distance, mean squared distance, hit fraction, 1 — probe placement.  A tensor on the tracer's device takes rt_visibility_device
        and returns a tensor."""
        self.InitFrame()
        return self.backend.visibility(points, samples, seed, firstIndex, mode)

    def ClosestPoints(self, points):
        """Beyond the reference: the nearest surface of the scene the next frame traces to each point (rt_closest_points) — which sphere
        or triangle, where on it, how far and on which side (+1 in front / outside, -1 behind / inside): signed-distance baking, pushing a
        probe out of a wall, snapping.  points: a RAY array or float32 (n, 8) with the point in origin and the search radius in tMax ->
        a CLOSEST array.  A tensor on the tracer's device takes rt_closest_points_device and returns a float32 (n, 16) tensor."""
        self.InitFrame()
        return self.backend.closest_points(points)

    def OverlapSphere(self, points, radius=None, maxResults=8, countAll=True):
        """Beyond the reference: Physics.OverlapSphere against the scene the next frame traces — the surfaces within `radius` of each
        point, nearest first (nearest.py, include/rt.h "K-nearest queries").  points as for ClosestPoints; radius None keeps the radii in
        tMax -> CLOSEST records (n, maxResults), the unused ones miss records, _reserved[0] of every record the number of ALL surfaces
        within the radius (countAll False: at most maxResults, and the search prunes by the last one listed)."""
        from . import nearest
        self.InitFrame()
        return nearest.nearest_k(self.backend, points, maxResults, radius, countAll)

    def SphereCast(self, rays, radius):
        """Beyond the reference: Physics.SphereCast against the scene the next frame traces — how far a ball of `radius` (a scalar or one
        value per ray) travels along each ray before it touches a sphere or a triangle's face, edge or vertex, and where (sweep.py,
        include/rt.h "sphere casts").  rays as for trace_rays -> HIT records with dst = the travel, hitPoint = the contact, normal = the
        contact normal and _reserved[0] = the contact feature."""
        from . import sweep
        self.InitFrame()
        return sweep.sphere_cast(self.backend, rays, radius)

    def RenderFeatures(self, frames: int = 1, firstFrame: int = None):
        """Beyond the reference: `frames` feature frames (rt_render_aov) of the scene and camera OnRenderImage would trace, accumulated into
        the two planes a denoiser takes beside the image.  Returns (albedo_coverage, normal_depth), each (rows, W, 4); frame indices
        continue from the planes' own count unless firstFrame is given.  The image and numRenderedFrames are left alone."""
        self.InitFrame()
        first = self.backend.aov_info()["framesAccumulated"] if firstFrame is None else firstFrame
        self.backend.render_aov(first, frames)
        return self.backend.read_aov(0), self.backend.read_aov(1)

    def Denoise(self, **params):
        """Beyond the reference: the step between resultTexture and the display blit (rt_denoise): the accumulated image filtered by the
        edge-avoiding A-trous transform, guided by the planes RenderFeatures accumulated.  Keywords as Tracer.denoise (none = the library's
        defaults).  Returns the denoised image (H, W, 4); the image, the planes and numRenderedFrames are left alone."""
        self.backend.denoise(**params)
        return self.backend.read_denoised()

    def DenoiseVariance(self, **params):
        """Beyond the reference: the variance-guided filter (rt_denoise_variance) of the accumulated image, or of the temporal colour with
        source=1, guided by the planes RenderFeatures accumulated: a per-pixel luminance variance estimated from the image scales the
        colour edge-stop.  Keywords as Tracer.denoise_variance (none = the library's defaults).  Returns (the denoised image (H, W, 4),
        the estimated variance (H, W)); the image, the planes and numRenderedFrames are left alone."""
        self.backend.denoise_variance(**params)
        return self.backend.read_denoised(), self.backend.read_variance()

    def Temporal(self, **params):
        """Beyond the reference: the step in front of Denoise for a moving camera (rt_temporal).  After a frame rendered from a fresh
        accumulation at the current pose and RenderFeatures at that pose, the previous result is reprojected into the new view and the
        new samples are blended in.  Keywords as Tracer.temporal (none = the library's defaults).  Returns the temporal colour
        (H, W, 4); the image, the planes and numRenderedFrames are left alone."""
        self.backend.temporal(**params)
        return self.backend.read_temporal()

    def Start(self):                                                              # RayTracingManager.cs:43-46
        self.numRenderedFrames = 0
        if self.backend is not None:
            self.backend.reset_accum()

    def OnRenderImage(self, frames: int = 1) -> np.ndarray:
        """RayTracingManager.cs:49-93 — trace + accumulate `frames` frames, return resultTexture (rows, W, 4)."""
        self.InitFrame()
        self.backend.render(self.numRenderedFrames, frames)
        self.numRenderedFrames += frames
        return self.backend.read_accum()


# ---- MeshSplitter (Assets/Scripts/Helpers/MeshSplitter.cs) ----------------------------------------------------------------
class _UBounds:
    """UnityEngine.Bounds in float32: stored as centre + extents (Bounds.cs of the public UnityCsReference):
    Bounds(c, size): extents = size*0.5; size = extents*2; min/max = centre -/+ extents;
    SetMinMax(mn, mx): extents = (mx-mn)*0.5, centre = mn + extents; Encapsulate(p) = SetMinMax(Min(min,p), Max(max,p));
    Contains(p): p >= centre-extents and p <= centre+extents on every axis (native AABB::IsInside — unpinned)."""
    __slots__ = ("center", "extents")

    def __init__(self, center, size):
        self.center = np.asarray(center, np.float32).copy()
        self.extents = (np.asarray(size, np.float32) * f32(0.5)).astype(np.float32)

    @property
    def size(self):
        return (self.extents * f32(2)).astype(np.float32)

    @property
    def min(self):
        return (self.center - self.extents).astype(np.float32)

    @property
    def max(self):
        return (self.center + self.extents).astype(np.float32)

    def set_min_max(self, mn, mx):
        self.extents = ((mx - mn) * f32(0.5)).astype(np.float32)
        self.center = (mn + self.extents).astype(np.float32)

    def encapsulate_points(self, pts):
        """Encapsulate a sequence of points one after the other (order matters in float32: centre/extents are re-derived
        after every point)."""
        for p in np.asarray(pts, np.float32).reshape(-1, 3):
            self.set_min_max(np.minimum(self.min, p), np.maximum(self.max, p))

    def contains(self, pts):
        pts = np.asarray(pts, np.float32)
        return np.all((pts >= self.min) & (pts <= self.max), axis=-1)


class MeshSplitter:
    """Restatement of MeshSplitter.cs:8-124: recursive 8-octant split until <= 48 triangles or depth 6; a triangle goes
    to the first octant (x, then y, then z loop order) that contains any of its vertices."""
    maxDepth = 6                # MeshSplitter.cs:8
    maxTrisPerChunk = 48        # MeshSplitter.cs:9

    @staticmethod
    def CreateSubMesh(triangles: np.ndarray, subMeshIndex: int, firstVertex=None) -> MeshChunk:
        """:35-63 — bounds start as a box of size 0.01 at the first vertex, then every vertex is encapsulated in order.
        `triangles` is the sub-mesh's triangle list (TRIANGLE[n]) in index-buffer order."""
        v0 = triangles["posA"][0] if firstVertex is None else firstVertex
        b = _UBounds(v0, np.full(3, 0.01, np.float32))
        pts = np.stack([triangles["posA"], triangles["posB"], triangles["posC"]], axis=1).reshape(-1, 3)
        b.encapsulate_points(pts)
        return MeshChunk(triangles.copy(), b, subMeshIndex)

    @staticmethod
    def CreateChunks(mesh) -> list:
        """:11-33 — `mesh` is a Mesh (vertices, normals, index buffer, sub-mesh ranges), or directly the sub-meshes'
        triangle lists [(TRIANGLE[n], subMeshIndex)] in sub-mesh order."""
        if isinstance(mesh, Mesh):
            sub_meshes = []
            for i, (start, count) in enumerate(mesh.subMeshes):
                idx = mesh.triangles[start:start + count].reshape(-1, 3)
                t = np.zeros(len(idx), TRIANGLE)
                for k, (pf, nf) in enumerate((("posA", "normalA"), ("posB", "normalB"), ("posC", "normalC"))):
                    t[pf] = mesh.vertices[idx[:, k]]
                    t[nf] = mesh.normals[idx[:, k]]
                sub_meshes.append((t, i))
        else:
            sub_meshes = mesh
        out = []
        for tris, idx in sub_meshes:
            MeshSplitter.Split(MeshSplitter.CreateSubMesh(tris, idx), out)
        return out

    @staticmethod
    def Split(chunk: MeshChunk, out: list, depth: int = 0):
        """:65-99"""
        tris = chunk.triangles
        if len(tris) > MeshSplitter.maxTrisPerChunk and depth < MeshSplitter.maxDepth:
            b = chunk.bounds
            q = (b.size / f32(4)).astype(np.float32)
            taken = np.zeros(len(tris), bool)
            for x in (-1, 1):
                for y in (-1, 1):
                    for z in (-1, 1):
                        if len(tris) - int(taken.sum()) > 0:
                            off = np.array([q[0] * f32(x), q[1] * f32(y), q[2] * f32(z)], np.float32)
                            split = _UBounds((b.center + off).astype(np.float32), (q * f32(2)).astype(np.float32))
                            sub = MeshSplitter.Extract(tris, taken, split, chunk.subMeshIndex)
                            if len(sub.triangles) > 0:
                                MeshSplitter.Split(sub, out, depth + 1)
        else:
            out.append(chunk)

    @staticmethod
    def Extract(tris: np.ndarray, taken: np.ndarray, split: "_UBounds", subMeshIndex: int) -> MeshChunk:
        """:101-124"""
        inside = split.contains(tris["posA"]) | split.contains(tris["posB"]) | split.contains(tris["posC"])
        pick = inside & ~taken
        new_bounds = _UBounds(split.center, split.size)
        sel = tris[pick]
        pts = np.stack([sel["posA"], sel["posB"], sel["posC"]], axis=1).reshape(-1, 3)
        new_bounds.encapsulate_points(pts)
        taken |= pick
        return MeshChunk(sel.copy(), new_bounds, subMeshIndex)
