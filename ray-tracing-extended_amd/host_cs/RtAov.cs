// RtAov.cs — the feature buffers of include/rt.h (rt_render_aov / rt_read_aov and their rt_multi forms; the DllImports are in
// RtNative.cs with the others): the plane indices and the accumulation state.  Checked against the C header by tests/test_aov_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    public static class RtAov
    {
        public const int Albedo = 0;                // RT_AOV_ALBEDO: (albedo.rgb, coverage)
        public const int NormalDepth = 1;           // RT_AOV_NORMAL_DEPTH: (normal.xyz, depth)
        public const int Count = 2;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtAovInfo                         // rt_aov_info, 24 B
    {
        public int framesAccumulated;               // feature frames in the planes
        public int lastSampleLanes;                 // lanes of a wave that shared a pixel's samples in the last launch (16, 4 or 1)
        public double lastKernelMs;                 // HIP-event time of the launches of the last rt_render_aov call
        public double totalKernelMs;                // sum since the planes were last zeroed
    }
}
