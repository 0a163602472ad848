// rt_stream.hpp — k_stream: the resumable-traversal megakernel.  Same per-pixel arithmetic as k_trace (rt_kernels.hpp),
// explicit per-lane mode (TRAV / SHADE / WAIT / DEAD) and a wave-level schedule built on ballots.
//
// k_trace binds an 8x8 tile to a wave and, per loop iteration, runs one complete closest-hit query for all 64 lanes
// before shading them: the wave pays for the longest traversal in it (measured on the 100k-triangle workload: 24 node
// steps executed per 9 needed) and for the slowest pixel of its tile.  Here
//   * traversal is *resumable*: a while-while burst ends as soon as `shade_threshold` lanes hold a complete query; the
//     stragglers keep cur / top / best hit / slab constants in registers, sit out the SHADE pass, and continue in the
//     next burst beside the other lanes' new rays — the wave no longer waits for its longest ray;
//   * inside a burst the node loop hands over to the leaf phase once fewer than `node_min` lanes still hold an internal
//     node (they wait one leaf phase) instead of running until the last descender reaches a leaf;
//   * SHADE (hit/miss shading, next bounce or next sample or next pixel, new ray, sphere loop, traversal reset) runs
//     for the lanes whose query is complete;
//   * a wave reserves `tiles_per_fetch` work items (frame, tile) per fetch — costliest tiles first — and a lane that
//     finishes its pixel of one tile moves on to its position in the next tile of the group; it idles (WAIT) only when
//     the group is exhausted.  (tile_sync = 0 refills lanes pixel by pixel from the global queue instead: the wave
//     loses its tile coherence and node-step utilisation drops from 37 % to 28 %.)
//
// Nothing about a pixel's own sequence of operations changes (same RNG chain, same closest-hit arithmetic, same
// tie-break), so the image is bit-identical to k_trace and to the oracle.
#pragma once
#include "rt_kernels.hpp"
#include "rt_types.hpp"             // CamRecord

namespace rtk {

struct StreamArgs {
    int shade_threshold;        // lanes waiting for SHADE that trigger it
    unsigned int total_pixels;  // tiles_x * tiles_y * 64 (tile-major enumeration, padded)
    int node_min;               // the node loop of a burst goes on while at least this many lanes hold an internal node (or no lane holds a leaf)
    int tiles_per_fetch;        // tile_sync: a wave reserves up to this many consecutive work items at a time; a lane that finishes its
                                // pixel of one moves on to its position in the next without waiting for the slower lanes
    int guide_div;              // ... as long as more than tiles_per_fetch * guide_div items are left in the launch's queue; below
                                // that the groups shrink to items_left / guide_div, down to single items (= waves of the launch x a factor)
    int tile_sync;              // 1: a wave takes a whole 8x8 tile at a time (coherent lanes), 0: lanes refill pixel by pixel
    int n16, n4, n1;            // tile_sync: the launch's frames as n16 groups of 16, then n4 groups of 4, then n1 single frames.  A work
                                // item is a sub-tile of 2x2 / 4x4 / 8x8 pixels in the 16 / 4 / 1 frames of a group: lane = (frame of the
                                // group, pixel of the sub-tile).  Frames are independent (frag :362 seeds by Frame), so the same pixel
                                // in 16 or 4 frames gives a wave rays that start almost identical and per-lane costs that are
                                // identically distributed
    int sample_lanes_log2;      // PHILOX instantiations: log2 S of the sample lanes per pixel (4 / 2 / 0 for NumRaysPerPixel >= 16 / >= 4 / else).
                                // The counter-based stream makes a pixel's samples independent, so a work item is a 2x2 / 4x4 / 8x8
                                // sub-tile of ONE frame whose pixels are spread over S lanes each: lane = (sample lane k, pixel of the
                                // sub-tile); lane k traces samples k, k + S, k + 2S, ... and the S partial sums meet in a fixed tree
                                // (the estimator of include/rt.h RT_RNG_PHILOX).  n1 = frames of the launch, n16 = n4 = 0
};

// kModeTravStrict: a traversal that evaluates the reference's chunk-box filter at every candidate (see "chunk filter" in k_stream); both
// traversal modes are the values <= 0 as signed integers: is_trav() is one compare
enum : uint32_t { kModeTrav = 0, kModeShade = 1, kModeDead = 2, kModeWait = 3, kModeTravStrict = 0xFFFFFFFFu };
__device__ __forceinline__ bool is_trav(uint32_t mode) { return (int)mode <= 0; }
constexpr uint32_t kNoPixel = 0xFFFFFFFFu;

struct StreamKernArgs { DeviceScene S; FrameArgs F; StreamArgs A; };     // k_stream's argument segment (fresh_kernargs, rt_kernels.hpp)
static_assert(alignof(StreamArgs) <= 8, "kernarg layout = struct layout");
// every by-value argument starts on the next multiple of 8 bytes in the kernarg segment; the struct view must put its members there too
// (tests/test_kernarg_layout_cpu.py reads the offsets back from the code object)
static_assert(offsetof(StreamKernArgs, F) == ((sizeof(DeviceScene) + 7) & ~size_t(7))
              && offsetof(StreamKernArgs, A) == ((offsetof(StreamKernArgs, F) + sizeof(FrameArgs) + 7) & ~size_t(7)), "kernarg layout = struct layout");

// k_cam_stream (rt_render_params): the camera of every frame of a launch is a CamRecord (rt_types.hpp)
struct StreamCamKernArgs { DeviceScene S; FrameArgs F; StreamArgs A; const CamRecord* cams; };     // k_cam_stream's argument segment
static_assert(offsetof(StreamCamKernArgs, A) == offsetof(StreamKernArgs, A)
              && offsetof(StreamCamKernArgs, cams) == ((offsetof(StreamCamKernArgs, A) + sizeof(StreamArgs) + 7) & ~size_t(7)), "kernarg layout = struct layout");

#ifndef RT_STREAM_WAVES
#define RT_STREAM_WAVES 7           // waves per SIMD of the PCG / f16-node instantiation (see below; 6 and 5 still build: -DRT_STREAM_WAVES=)
#endif
#ifndef RT_STREAM_WAVES_PHILOX
#define RT_STREAM_WAVES_PHILOX 5    // (six waves = 80 VGPRs: 34 of them spilled, 13.9 against 16.9 Grays/s — round 4, one box, interleaved)
#endif
constexpr int stream_waves(bool count, bool philox, bool h, bool tri) { return count ? 3 : !tri ? 6 : philox ? RT_STREAM_WAVES_PHILOX : !h ? 5 : RT_STREAM_WAVES; }     // (counting build: 47 counters in registers)
// Which instantiation holds how many: PCG / f16 nodes seven (72 VGPRs); PCG / f32 nodes five (94) and Philox with triangles five (96): the register
// diet below does not bring either under 80 without scratch; the sphere-only ones six as before (PCG 75; Philox 80, of which k_stream keeps one
// spilled VGPR, 8 B of scratch — measured with it: 32.6 -> 35.1 Grays/s against five waves, see below — and k_cam_stream none).


// Waves per SIMD.  The kernel hides its memory and LDS latencies with resident waves.  Round 2 chose five (96 VGPRs; six = 80 VGPRs spilled
// 26 dwords and lost: 14.18 against 14.70 Grays/s).  Round 4: compiled without structurizing uniform regions (__graft_entry__.py
// STREAM_TU_FLAGS) the PCG / f16-node instantiation fits 80 VGPRs WITHOUT scratch, and six waves per SIMD — with an LDS stack of <= 24
// entries per lane, so that six workgroups fit a CU — measure 18.3 against 17.1 Grays/s at five on the 100k-triangle workload, 16.2
// against 15.1 on the million-triangle one (seven: 72 VGPRs + 5 dwords of scratch, 17.2; eight: 15.1).  The Philox instantiation spills
// at 80 VGPRs (14 dwords: 13.1 against 15.8 Grays/s) and stays at five, like the f32-node and the counting instantiations.
// Seven waves: 72 VGPRs and NO scratch, since three per-lane registers went away — the f16 slab keeps its three node offsets in one
// register (RaySlabT<true>::sets, rt_kernels.hpp: one more VALU per node step) and bounce shares `sample`'s register in the PCG
// instantiations as it always did in the Philox ones.  Seven workgroups per CU need an LDS stack of <= 21 entries per lane (7 x 22,016 B
// of the 160 KiB); the stack guard is a scalar test while no lane can be near the end of that part (`ub`, rt_stream_body.hpp).  One box,
// five interleaved pairs, 16 frames each (profiles/ab_seven_waves.txt): 20.65-20.76 against 19.76-19.94 Grays/s at six on the 100k-triangle
// workload (+4.2 %), 17.9 against 17.3 on the million-triangle one (medians; its runs scatter more at seven).
// TRI = false: the instantiation for scenes without triangles (spheres only) — no traversal state, no burst; 75 / 86 VGPRs by itself (PCG / Philox),
// compiled for six waves per SIMD: 36.4 -> 39.3 (PCG; k_trace's sphere instantiation stays ahead at 41.7) and 32.6 -> 35.1 Grays/s (Philox)
// on the sphere workload, eight waves (64 VGPRs, scratch): 37.6 / 29.7.
template <bool COUNT, bool PHILOX = false, bool H = false, bool TRI = true>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(stream_waves(COUNT, PHILOX, H, TRI), stream_waves(COUNT, PHILOX, H, TRI)))) void k_stream(DeviceScene S, FrameArgs F, StreamArgs A)
{
    constexpr bool CAMS = false;
#include "rt_stream_body.hpp"
}

// k_stream with a per-frame camera table (rt_render_params: a camera that moves between the frames of one launch).  The same body and the
// same waves per SIMD as its k_stream twin; only the non-counting instantiations exist (the counting build renders such a run frame by frame).
template <bool PHILOX, bool H, bool TRI>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(stream_waves(false, PHILOX, H, TRI), stream_waves(false, PHILOX, H, TRI)))) void k_cam_stream(DeviceScene S, FrameArgs F, StreamArgs A, const CamRecord* cams)
{
    constexpr bool COUNT = false, CAMS = true;
    (void)cams;                 // (read through the kernarg view where it is used: StreamCamKernArgs)
#include "rt_stream_body.hpp"
}

} // namespace rtk
