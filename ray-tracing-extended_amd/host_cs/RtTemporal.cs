// RtTemporal.cs — temporal reprojection of include/rt.h (rt_temporal / rt_read_temporal / rt_denoise_temporal and their rt_multi
// forms; the DllImports are in RtNative.cs with the others): the parameters of a call and the state of the step.  Checked against
// the C header by tests/test_temporal_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public struct RtTemporalParams                  // rt_temporal_params, 32 B
    {
        public int maxHistory;                      // 1..4096
        public float depthTolerance;                // relative to the reprojected point's distance; finite and > 0
        public float normalTolerance;               // on |nc - G'.xyz|; finite and > 0
        public int _reserved0, _reserved1, _reserved2, _reserved3, _reserved4;

        /// RT_TEMPORAL_DEFAULT_* of include/rt.h (what a null pointer means in C)
        public static RtTemporalParams Defaults
        {
            get { return new RtTemporalParams { maxHistory = 32, depthTolerance = 0.05f, normalTolerance = 0.5f }; }
        }
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtTemporalInfo                    // rt_temporal_info, 32 B
    {
        public int calls;                           // since the history was last dropped
        public int width, height;
        public int _reserved;
        public double lastKernelMs;                 // HIP-event time of the last call's launch
        public double totalKernelMs;
    }
}
