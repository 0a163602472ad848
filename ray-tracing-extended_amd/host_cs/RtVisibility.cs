// RtVisibility.cs — the two structs of the visibility gathers of include/rt.h (rt_visibility and its device and rt_multi forms; the
// DllImports are in RtNative.cs with the others, a point is RtQuery.cs' RtRay with the normal in its direction field and the reach in
// its maxDistance): the parameters of a call and the state of the last one.  Plain sequential layouts, checked field by field against
// the C header by tests/test_visibility_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtVisibilityParams         // rt_visibility_params, 32 B
    {
        public int samples;                         // N, 1..65536: directions per point
        public uint seed;                           // second key word of the Philox stream
        public uint firstIndex;                     // point i of the call has stream index firstIndex + i
        public int mode;                            // 0 = RT_VIS_COSINE, 1 = RT_VIS_SH9 (three float4 per point), 2 = RT_VIS_DISTANCE
        public fixed int _reserved[4];              // must be 0
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtVisibilityInfo                  // rt_visibility_info, 32 B
    {
        public int samples;                         // of the last call
        public int lastSampleLanes;                 // lanes of a wave that shared a point's samples in the last launch (16, 4 or 1)
        public int calls, mode;                     // calls so far / the last call's mode
        public double lastKernelMs, totalKernelMs;  // HIP-event time of the launches of the last host-entry call / summed
    }
}
