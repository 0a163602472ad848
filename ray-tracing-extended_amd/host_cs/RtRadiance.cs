// RtRadiance.cs — the two structs of the radiance queries of include/rt.h (rt_trace_radiance and its device and rt_multi forms; the
// DllImports are in RtNative.cs with the others, the rays are RtQuery.cs' RtRay): the parameters of a call and the state of the last one.
// Plain sequential layouts, checked field by field against the C header by tests/test_radiance_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct RtRadianceParams           // rt_radiance_params, 32 B
    {
        public int samples;                         // N, 1..65536: independent runs of Trace per ray
        public uint seed;                           // second key word of the Philox stream (what Frame is for a frame)
        public uint firstIndex;                     // ray i of the call has stream index firstIndex + i
        public fixed int _reserved[5];              // must be 0
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtRadianceInfo                    // rt_radiance_info, 32 B
    {
        public int samples;                         // of the last call
        public int lastSampleLanes;                 // lanes of a wave that shared a ray's samples in the last launch (16, 4 or 1)
        public int calls, _reserved;
        public double lastKernelMs, totalKernelMs;  // HIP-event time of the launches of the last host-entry call / summed
    }
}
