// RtClosest.cs — the two structs of the closest-point queries of include/rt.h (rt_closest_points and its device and rt_multi forms; the
// DllImports are in RtNative.cs with the others, a point is RtQuery.cs' RtRay with the position in its origin and the search radius in
// its tMax): the record of a point's nearest surface and the state of the last call.  Plain sequential layouts, checked field by field
// against the C header by tests/test_closest_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtClosest                  // rt_closest, 64 B
    {
        public float dst;                           // unsigned distance to `point`; +inf when nothing lies within the radius
        public fixed float point[3];                // the closest point of the closest primitive
        public fixed float normal[3];               // the shading normal there, as RtHit.normal
        public int kind;                            // 0 none, 1 sphere, 2 triangle
        public int primitive;                       // as in RtHit
        public int chunk;
        public int mesh;
        public float u, v;                          // triangle: point = A + (B - A) * u + (C - A) * v; else 0
        public int side;                            // +1 in front of the triangle / outside the sphere, -1 behind / inside, 0 on it or a miss
        public fixed int _reserved[2];
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtClosestInfo                     // rt_closest_info, 40 B
    {
        public int calls;                           // calls so far
        public int _reserved;
        public double lastKernelMs, totalKernelMs;  // HIP-event time of the launches of the last host-entry call / summed
        public ulong lastNodeSteps, lastPrimTests;  // option "closest_count" = 1: node steps and primitive tests of the last call; else 0
    }
}
