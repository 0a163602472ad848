// RtHits.cs — the three structs of the multi-hit ray queries of include/rt.h (rt_trace_hits and its device and rt_multi forms; the
// DllImports are in RtNative.cs with the others, a ray is RtQuery.cs' RtRay): the params of a call, one of a ray's maxHits records and
// the state of the last call.  Plain sequential layouts, checked field by field against the C header by tests/test_hits_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtHitsParams               // rt_hits_params, 32 B
    {
        public int maxHits;                         // records per ray, 1..8
        public int mode;                            // 0 front faces and sphere entries, 1 back faces and sphere exits as well
        public int countAll;                        // 1: hitCount counts every hit below tMax, not min(hits, maxHits)
        public fixed int _reserved[5];              // must be 0
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtMultiHit                 // rt_multihit, 64 B
    {
        public float dst;                           // +inf in an empty record
        public fixed float hitPoint[3];             // origin + direction * dst
        public fixed float normal[3];               // as RtHit.normal; not flipped for a back hit
        public int kind;                            // 0 none (an empty record), 1 sphere, 2 triangle
        public int primitive;                       // as in RtHit
        public int chunk;
        public int mesh;
        public float u, v;                          // triangle: RayTriangle's u, v; else 0
        public int side;                            // +1 front face / sphere entry, -1 back face / sphere exit, 0 in an empty record
        public int hitCount;                        // the same in all records of a ray
        public int _reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtHitsInfo                        // rt_hits_info, 32 B
    {
        public int calls;                           // calls so far
        public int lastMaxHits, lastMode, lastCountAll;     // the params of the last call, defaults filled in
        public double lastKernelMs, totalKernelMs;  // HIP-event time of the launches of the last host-entry call / summed
    }
}
