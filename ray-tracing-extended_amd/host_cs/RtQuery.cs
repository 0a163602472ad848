// RtQuery.cs — the two structs of the ray-query entry points of include/rt.h (rt_trace_rays / rt_occluded and their device and
// rt_multi forms; the DllImports are in RtNative.cs with the others).  Plain sequential layouts of primitive fields and fixed buffers,
// checked field by field against the C header by tests/test_ray_query_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtRay                      // rt_ray, 32 B
    {
        public fixed float origin[3];
        public float tMax;                          // only hits with dst < tMax count; +inf = unbounded; <= 0 or NaN = a miss
        public fixed float direction[3];            // not normalised: dst is in units of |direction|
        public int _reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtHit                      // rt_hit, 64 B — CalculateRayCollision (RayTracing.shader:256-297)
    {
        public float dst;                           // +inf on a miss
        public fixed float hitPoint[3];
        public fixed float normal[3];
        public int kind;                            // 0 none, 1 sphere, 2 triangle
        public int primitive;                       // sphere: index in the sphere buffer; triangle: index in the triangle buffer; else -1
        public int chunk;                           // triangle: its MeshInfo index; else -1
        public int mesh;                            // triangle of a local-mesh scene: its mesh index; else -1
        public float u, v;                          // triangle: barycentrics (w = 1 - u - v); else 0
        public fixed int _reserved[3];
    }
}
