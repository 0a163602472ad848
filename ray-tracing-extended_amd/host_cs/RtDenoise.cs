// RtDenoise.cs — the denoiser of include/rt.h (rt_denoise / rt_read_denoised and their rt_multi forms; the DllImports are in
// RtNative.cs with the others): the parameters of a call and the state of the last one.  Checked against the C header by
// tests/test_denoise_cpu.py.
using System.Runtime.InteropServices;

namespace RtMi355x
{
    [StructLayout(LayoutKind.Sequential)]
    public struct RtDenoiseParams                   // rt_denoise_params, 32 B
    {
        public int iterations;                      // 1..6; pass i uses tap spacing 2^i
        public int demodulate;                      // 0 / 1
        public float sigmaColour, sigmaNormal, sigmaDepth;      // each finite and > 0
        public int _reserved0, _reserved1, _reserved2;

        /// RT_DENOISE_DEFAULT_* of include/rt.h (what a null pointer means in C)
        public static RtDenoiseParams Defaults
        {
            get { return new RtDenoiseParams { iterations = 5, demodulate = 0, sigmaColour = 16.0f, sigmaNormal = 1.0f, sigmaDepth = 0.5f }; }
        }
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtVDenoiseParams                  // rt_vdenoise_params, 32 B (the variance-guided filter: rt_denoise_variance)
    {
        public int iterations;                      // 1..6; pass i uses tap spacing 2^i
        public int demodulate;                      // 0 / 1
        public int source;                          // 0 = resultTexture, 1 = the temporal plane
        public float sigmaLuminance, sigmaNormal, sigmaDepth;   // each finite and > 0
        public int _reserved0, _reserved1;          // must be 0

        /// RT_VDENOISE_DEFAULT_* of include/rt.h and source 0 (what a null pointer means in C)
        public static RtVDenoiseParams Defaults
        {
            get { return new RtVDenoiseParams { iterations = 3, demodulate = 1, source = 0, sigmaLuminance = 8.0f, sigmaNormal = 0.25f, sigmaDepth = 0.5f }; }
        }
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtVDenoiseInfo                    // rt_vdenoise_info, 32 B
    {
        public int iterations;                      // of the last call
        public int source;                          // of the last call
        public int width, height;
        public double lastKernelMs;                 // HIP-event time of the last call's launches
        public double totalKernelMs;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtDenoiseInfo                     // rt_denoise_info, 32 B
    {
        public int iterations;                      // of the last call
        public int demodulate;                      // of the last call
        public int width, height;
        public double lastKernelMs;                 // HIP-event time of the last call's launches
        public double totalKernelMs;
    }
}
