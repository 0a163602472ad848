/*
 * rt.h — C-ABI of the MI355X-native path tracer (drop-in for the per-pixel ray-trace path of
 * MaxLayar/Ray-Tracing-Extended).
 *
 * The reference tracer sits behind Unity's material-property API; its only caller is
 * RayTracingManager (Assets/Scripts/RayTracingManager.cs:49-187).  Every entry point below names the
 * reference call it replaces.  All structs are plain little-endian PODs; buffer strides are the
 * reference's own Marshal.SizeOf strides (Assets/Scripts/Helpers/ShaderHelper.cs:106,124):
 *
 *   RayTracingMaterial 64 B   Assets/Scripts/Data Types/RayTracingMaterial.cs:13-19, RayTracing.shader:67-76
 *   Sphere             80 B   Assets/Scripts/Data Types/Sphere.cs:5-7,              RayTracing.shader:78-83
 *   Triangle           72 B   Assets/Scripts/Data Types/Triangle.cs:8-14,           RayTracing.shader:85-89
 *   MeshInfo           96 B   Assets/Scripts/Data Types/MeshInfo.cs:5-9,            RayTracing.shader:91-98
 *
 * No torch / C++ types cross this boundary.  Errors are int status codes (0 = ok); the message of the
 * last failure is available from rt_last_error().  Nothing throws or aborts across the ABI.
 * A context is not thread-safe (the reference is single-threaded: Unity main thread in OnRenderImage).
 * The library is GPU-only: rt_create() fails when no HIP device is present — there is no CPU fallback.
 */
#ifndef RT_H_
#define RT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- buffer element layouts (accepted verbatim from the reference host) ------------------------- */

typedef struct rt_material {            /* 64 B */
    float   colour[4];
    float   emissionColour[4];
    float   specularColour[4];
    float   emissionStrength;
    float   smoothness;
    float   specularProbability;
    int32_t flag;                       /* 0 None, 1 CheckerPattern, 2 InvisibleLight (RayTracingMaterial.cs:6-11) */
} rt_material;

typedef struct rt_sphere {              /* 80 B */
    float       position[3];
    float       radius;
    rt_material material;
} rt_sphere;

typedef struct rt_triangle {            /* 72 B */
    float posA[3], posB[3], posC[3];
    float normalA[3], normalB[3], normalC[3];
} rt_triangle;

typedef struct rt_meshinfo {            /* 96 B */
    uint32_t    firstTriangleIndex;
    uint32_t    numTriangles;
    rt_material material;
    float       boundsMin[3];
    float       boundsMax[3];
} rt_meshinfo;

/* ---- on-device geometry pipeline (optional) -----------------------------------------------------------------
 * The reference transforms every mesh to world space on the CPU and re-uploads the scene every frame
 * (RayTracedMesh.cs:36-84, RayTracingManager.cs:135-164; TODO at RayTracedMesh.cs:37).  With these two layouts the
 * local-space chunks are uploaded once and a frame only sends one transform per mesh.                       */
typedef struct rt_mesh_transform {      /* 40 B: transform.position / rotation (x,y,z,w) / lossyScale (RayTracedMesh.cs:38-40) */
    float position[3];
    float rotation[4];
    float lossyScale[3];
} rt_mesh_transform;

typedef struct rt_local_chunk {         /* 80 B: one MeshChunk of RayTracedMesh.localChunks (MeshChunk.cs:6-17) */
    uint32_t    firstTriangleIndex;     /* into the local triangle buffer                                        */
    uint32_t    numTriangles;
    uint32_t    meshIndex;              /* which rt_mesh_transform moves it                                      */
    uint32_t    _reserved;
    rt_material material;               /* RayTracedMesh.GetMaterial(chunk.subMeshIndex), RayTracedMesh.cs:96-99 */
} rt_local_chunk;

/* ---- uniforms ------------------------------------------------------------------------------------
 * One POD holding exactly what RayTracingManager pushes with Material.Set{Int,Float,Vector,Matrix,Color}
 * (RayTracingManager.cs:113-123,131-132) plus the three Unity built-ins the shader reads
 * (_ScreenParams.xy, _WorldSpaceCameraPos, _WorldSpaceLightPos0: RayTracing.shader:359,378,247).     */

enum {
    RT_RNG_PCG = 0,                     /* RayTracing.shader:193-204 — the reference's stream, the parity mode            */
    RT_RNG_PHILOX = 1                   /* the LATENCY mode: counter-based Philox4x32-10 (Salmon et al., SC'11).  NOT the reference's
                                           stream: different noise, same expectation.  A single frame finishes sooner in it (a pixel's samples
                                           spread over 16 lanes: 16.3 against 18.3 ms on the headline workload, round 4); in launches of many
                                           frames the PCG stream is the faster one (18.3 against 15.8 Grays/s: the generator costs more
                                           instructions than the chain's hash and its kernel keeps five waves per SIMD instead of six).  The reference chains one PCG state through every
                                           sample and bounce of a pixel (RayTracing.shader:362,374-385), which forbids spreading a
                                           pixel's samples over lanes; here every draw is addressed by what it is for:
                                             key     = (pixelIndex, Frame)                     (frag :360-362)
                                             counter = (block, sample, 0, 0)
                                             block 0               the sample's camera ray: words 0..3 = the four draws of frag
                                                                   :377,380 in the shader's order
                                             blocks 1+2b, 2+2b     the hit at loop index b of Trace (:305): the eight draws of
                                                                   :325-339 in the shader's order, words 0..3 of the first block,
                                                                   then of the second (a bounce that draws nothing leaves them unused)
                                           and the estimator's sum over the NumRaysPerPixel samples (:384) is a fixed tree instead of a
                                           left-to-right chain: sample s goes to sub-stream s mod S, S = 16 / 4 / 1 for NumRaysPerPixel
                                           >= 16 / >= 4 / else; a sub-stream adds its samples in increasing order starting from 0;
                                           the S sub-sums are added pairwise, (k, k+1) for even k, then (k, k+2) for k = 0 mod 4, ...;
                                           the root is divided by NumRaysPerPixel (:387).  Scatter, Russian roulette and everything
                                           else are the reference's.  On the device the S sub-streams of a pixel are S lanes of one
                                           wave (k_stream's Philox instantiation), the tree is an in-wave reduction                  */
};
enum {
    RT_INTERSECT_FLAT_CHUNKS = 0,       /* literal reference result: a triangle counts only if its chunk's
                                           RayBoundingBox test passes (RayTracing.shader:276-294).  k_stream applies the test to a
                                           ray's answer (the closest triangle over all chunks) and traces the ray again, with the
                                           test at every candidate, only if the answer fails it: same result, 8-10 % faster       */
    RT_INTERSECT_BRUTE = 1              /* no chunk cull: closest hit over all triangles                  */
};

typedef struct rt_params {
    int32_t width, height;              /* _ScreenParams.xy (render-target size)                          */
    int32_t maxBounceCount;             /* "MaxBounceCount"  (loop is inclusive: B+1 casts, shader :305)  */
    int32_t numRaysPerPixel;            /* "NumRaysPerPixel"                                             */
    float   defocusStrength;            /* "DefocusStrength"                                             */
    float   divergeStrength;            /* "DivergeStrength"                                             */
    float   viewParams[3];              /* "ViewParams" = (planeWidth, planeHeight, focusDistance)       */
    float   camLocalToWorld[16];        /* "CamLocalToWorldMatrix", row-major m[row*4+col]               */
    float   worldSpaceCameraPos[3];     /* _WorldSpaceCameraPos                                          */
    float   worldSpaceLightPos0[3];     /* _WorldSpaceLightPos0.xyz (= -forward of the directional light) */
    int32_t environmentEnabled;         /* "EnvironmentEnabled"                                          */
    float   groundColour[4];            /* "GroundColour"     (already in the space the shader sees)     */
    float   skyColourHorizon[4];        /* "SkyColourHorizon"                                            */
    float   skyColourZenith[4];         /* "SkyColourZenith"                                             */
    float   sunFocus;                   /* "SunFocus"                                                    */
    float   sunIntensity;               /* "SunIntensity"                                                */
    int32_t rngMode;                    /* RT_RNG_*                                                      */
    int32_t intersectMode;              /* RT_INTERSECT_*                                                */
} rt_params;

/* ---- statistics (the reference exposes numRenderedFrames / numMeshChunks / numTriangles,
 *      RayTracingManager.cs:25-28,156-157; the work counters are new)                                 */
typedef struct rt_stats {
    int32_t  numRenderedFrames;         /* frames accumulated so far                                     */
    int32_t  numMeshChunks;
    int32_t  numTriangles;
    int32_t  numSpheres;
    int32_t  numBvhNodes;
    int32_t  bvhMaxStack;               /* worst-case traversal stack depth of the built BVH             */
    uint64_t rays;                      /* CalculateRayCollision invocations of the last render call     */
    uint64_t sphereTests;               /* the remaining counters: rt_render_counting only               */
    uint64_t nodeVisits;                /* BVH nodes fetched                                             */
    uint64_t triTests;
    uint64_t hits;                      /* rays that hit something                                       */
    uint64_t phaseLanes[5];             /* active lanes summed over executions of phase k: 0 BVH node step,  */
    uint64_t phaseExecs[5];             /* 1 triangle test, 2 hit shading, 3 environment, 4 camera ray;      */
                                        /* lane utilisation of phase k = phaseLanes[k] / (64*phaseExecs[k])  */
    double   lastKernelMs;              /* HIP-event time of the last trace(+accumulate) launch          */
    double   totalKernelMs;             /* sum over launches since rt_reset_accum                        */
    double   lastGeometryMs;            /* HIP-event time of the last on-device transform + bounds + re-layout + refit */
    double   lastDisplayMs;             /* HIP-event time of the last linear -> sRGB8 display kernel     */
    int32_t  lastFramesPerLaunch;       /* frames traced per k_trace launch in the last rt_render (1 = frame by frame) */
    int32_t  autoKernel;                /* kernel the automatic choice picked for single-frame launches (-1 = not decided yet / not automatic) */
    int32_t  lastKernel;                /* kernel that ran the last launch: 0 k_trace, 1 k_stream, 2 k_stream with a per-frame camera table, 4 flat twin */
    int32_t  lastFramesInterleaved;     /* k_stream: frames interleaved in a wave by the last launch (1, 4 or 16)        */
    double   lastBvhBuildMs;            /* last BVH build: HIP-event time of the device builder (sort + PLOC + collapse + records), */
                                        /* or host wall time of the binned-SAH builder                                   */
    float    refitAreaRatio;            /* internal box area after the last refit / right after the last build           */
    float    bvhInternalArea;           /* sum of the half-areas of all child boxes right after the last build (tree quality) */
    int32_t  bvhBuiltOnDevice;          /* 1: the current tree came from the device builder                              */
    int32_t  bvhBuilds;                 /* builds since rt_create                                                        */
    int32_t  bvhRebuilds;               /* ... of which triggered by a refit that had inflated the tree                  */
    int32_t  bvhRepads;                 /* times the box padding was widened on the device (a ray origin moved beyond the magnitude the
                                           boxes were padded for: refit of the existing tree, no rebuild, no re-upload)   */
    int32_t  lastSampleLanes;           /* Philox mode: lanes of a wave that shared a pixel's samples in the last launch (16, 4 or 1) */
    int32_t  queuedLaunches;            /* launches the rt_submit_frame queue has made since rt_reset_accum                */
    uint64_t regionExecs[32];           /* rt_render_counting, k_stream: wave-level executions of its regions, in the order of csrc/rt_kernels.hpp      */
                                        /* RT_REGION_LIST (loop, fetch, shade, hit, ...).  Multiplied with the regions' static VALU counts (from the code */
                                        /* object's assembly, tools/static_valu.py) they give the launch's VALU instruction count without a profiler:      */
                                        /* bench.py roofline.valu_model                                                                                   */
    uint32_t primaryLists[4];           /* camera rays' candidate lists of the last build (k_stream, static camera): pixels whose camera rays  */
                                        /* start from <= 4 leaves bounded by a common triangle / from an unbounded list / certainly miss         */
                                        /* everything / start at the root (no list)                                                              */
    int32_t  primaryListBuilds;         /* times the lists were built since rt_create                                                            */
    int32_t  _reserved;
    double   lastPrimaryListsMs;        /* HIP-event time of the last build of the lists                                                         */
} rt_stats;

typedef struct rt_ctx rt_ctx;

/* Lifetime.  Replaces ShaderHelper.InitMaterial / Release (ShaderHelper.cs:147-158,266-289;
 * RayTracingManager.cs:98-99,190-194).  device = HIP device ordinal.  Returns NULL on failure
 * (message retrievable with rt_last_error(NULL)).                                                      */
rt_ctx*     rt_create(int device);
void        rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);

/* Optional: run on a caller-owned hipStream_t (pass as void*).  NULL restores the context's own stream.  The switch is ordered: work the
 * context enqueued on the outgoing stream completes before anything it enqueues on the incoming one (an event recorded on the outgoing
 * stream, waited for by the incoming one), so a device query left running on a caller's stream is never overtaken by the context's next
 * upload, geometry pass or render.                                                                                                   */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);

/* Uniform upload.  Replaces SetShaderParams + UpdateCameraParams (RayTracingManager.cs:111-133).
 * Changing width/height re-creates (zeroes) the accumulation target, as ShaderHelper.CreateRenderTexture
 * does (ShaderHelper.cs:186-205).                                                                     */
int rt_set_params(rt_ctx* ctx, const rt_params* params);

/* Buffer upload = copy (caller may free immediately); n == 0 is legal.  Replaces
 * ShaderHelper.CreateStructuredBuffer + Material.SetBuffer/SetInt
 * (RayTracingManager.cs:159-163 "Triangles"/"AllMeshInfo"/"NumMeshes", :184-186 "Spheres"/"NumSpheres").
 * The library re-lays-out triangles and builds its BVH lazily at the next render.
 * With option "device_geometry" = 1 (rt_set_option) `tris` may lie in device memory: see the option.   */
int rt_upload_spheres  (rt_ctx* ctx, const rt_sphere*   spheres,  int n);
int rt_upload_triangles(rt_ctx* ctx, const rt_triangle* tris,     int n);
int rt_upload_meshinfo (rt_ctx* ctx, const rt_meshinfo* meshinfo, int n);

/* On-device geometry pipeline.  rt_upload_local_meshes replaces rt_upload_triangles + rt_upload_meshinfo: local-space
 * triangles (reference layout, 72 B) and their chunks; rt_set_mesh_transforms sends the n_meshes poses.  The library
 * transforms to world space on the GPU (rot * Scale(p, lossyScale) + pos; normals rot * n — RayTracedMesh.cs:86-94),
 * recomputes the chunks' world AABBs (:74-82), and refits its BVH; the image is bit-identical to uploading the
 * host-transformed buffers.  rt_read_world_geometry returns what the reference's CreateMeshes would have uploaded
 * (n_tris rt_triangle, n_chunks rt_meshinfo).                                                                  */
int rt_upload_local_meshes(rt_ctx* ctx, const rt_triangle* local_tris, int n_tris,
                           const rt_local_chunk* chunks, int n_chunks, int n_meshes);
int rt_set_mesh_transforms(rt_ctx* ctx, const rt_mesh_transform* transforms, int n_meshes);
int rt_read_world_geometry(rt_ctx* ctx, rt_triangle* tris_out, int n_tris, rt_meshinfo* meshinfo_out, int n_chunks);

/* Tuning knobs; the image never depends on them (tested bitwise).
 *   "kernel"          -1 = automatic (default): the first frames after a scene / camera change time k_trace and k_stream on
 *                     ordinary frames of the render and the faster one takes the rest; 0 = tile-per-wave megakernel k_trace,
 *                     1 = k_stream (resumable traversal, stragglers deferred; the only kernel of the Philox mode)
 *                     k_stream takes at most 65000 rays per pixel per frame and 32000 bounces (sample and bounce counters share one register);
 *                     a PCG frame with more is k_trace's whatever this option says (rt_stats.lastKernel = 0), a Philox frame with more is refused
 *   "max_leaf"        triangles per BVH leaf, 1..4 (default 2)
 *   "bvh_bins", "bvh_cost_exp", "bvh_reinsert"   BVH builder: SAH bins per axis (32); exponent, in percent, of the triangle
 *                     count in the SAH's subtree-cost model (100); passes of insertion-based optimisation of the binary tree (0:
 *                     measured -3 % node visits per ray but no fewer wave-level steps)
 *   "bvh_collapse", "bvh_node_cost"   host builder: how the binary SAH tree becomes 4-wide nodes — 0 = greedy, open the child of largest
 *                     area (default); 1 = cost-driven dynamic programme that also forms the leaves; 2 = the same over the split search's
 *                     leaves; with a node step costing bvh_node_cost percent of a triangle test (130)
 *   "stream_stack"    k_stream: traversal-stack entries per lane kept in LDS; a BVH whose worst case is deeper spills the rest to global memory.
 *                     0 (default) = automatic: 21 for the seven-waves-per-SIMD instantiation (PCG stream, f16 nodes: seven workgroups per CU), 30 for
 *                     the five-wave ones (Philox mode, f32 nodes, counting build)
 *   "full_sort"       1 = sort all four children of a node by entry distance, 0 = nearest first only (default)
 *   "tile_lpt"        k_trace: 1 = hand tiles out costliest first, by the costs the previous launch measured (default), 0 = in order
 *   "frame_batch"     k_trace: frames traced per launch by rt_render (0 = auto: as many as fit 4 GiB, at most 256; 1 = one per launch)
 *   "lds_stack"       k_trace: traversal-stack entries kept in LDS, deeper ones spill to global memory (0 = all in LDS)
 *   "radiance_slice"  rt_trace_radiance: rays per launch and per staging slice, 1..4194304 (default 4194304, the ray queries' slice); the
 *                     result never depends on it
 *   "gather_slice"    rt_gather: points per launch and per staging slice, 1..4194304 (default 1048576: an SH9 result is 144 B per point);
 *                     the result never depends on it
 *   "visibility_slice" rt_visibility: points per launch and per staging slice, 1..4194304 (default 4194304, the ray queries' slice);
 *                     the result never depends on it
 *   "closest_slice"   rt_closest_points: points per launch and per staging slice, 1..4194304 (default 4194304); the result never
 *                     depends on it
 *   "closest_count"   rt_closest_points: 1 = the counting build of the kernel, which fills rt_closest_info.lastNodeSteps / lastPrimTests
 *                     (default 0: those stay 0); the results are the same bits
 *   "closest_k"       K, 1..8 (RT_HITS_MAX), default 1: rt_closest_points, rt_closest_points_device and rt_multi_closest_points write K
 *                     rt_closest records per point, the K nearest candidates in order: see "K-nearest queries" below.  Other values are
 *                     refused with -2 and nothing changes.  Every other call ignores it
 *   "closest_all"     0 (default) or 1: with 1 the count those three calls report is the number of ALL candidates within the radius and the
 *                     search is bounded by the radius alone ("K-nearest queries").  Other values are refused with -2 and nothing changes.
 *                     Every other call ignores it.  At "closest_k" = 1 and "closest_all" = 0 the three calls are exactly what they were
 *   "closest_box"     0 (default) or 1: with 1 rt_closest_points, rt_closest_points_device and rt_multi_closest_points read each input as an
 *                     axis-aligned box (origin = centre, direction = half-extents) and answer for the candidates that touch it: see
 *                     "box overlap queries" below.  Other values are refused with -2 and nothing changes.  Every other call ignores it;
 *                     at 0 the three calls are exactly what they were.  Refused with -2 at 1 while "closest_capsule" is 1
 *   "closest_capsule" 0 (default) or 1: with 1 the same three calls read each input as a segment (origin = P0, direction = P1 - P0,
 *                     tMax = the reach) and answer the K-nearest question for it: see "capsule overlap queries" below.  Other values, and 1
 *                     while "closest_box" is 1, are refused with -2 and nothing changes.  Every other call ignores it; at 0 the three
 *                     calls are exactly what they were
 *   "hits_slice"      rt_trace_hits: rays per launch and per staging slice, 1..4194304 (default 262144: at most 128 MiB of staged records
 *                     at maxHits = 8); the result never depends on it
 *   "sweep"           0 (default) = the ray queries trace rays; 1 = rt_trace_rays, rt_trace_rays_device, rt_multi_trace_rays, rt_occluded,
 *                     rt_occluded_device and rt_multi_occluded answer for a BALL swept along each ray, its radius the float whose bits are
 *                     rt_ray._reserved: see "sphere casts" below.  Other values are refused with -2.  rt_trace_hits, the radiance,
 *                     gather, visibility and closest-point calls and every frame ignore it; at 0 nothing reads rt_ray._reserved
 *   "hits_sweep"      0 (default) or 1: with 1 rt_trace_hits, rt_trace_hits_device and rt_multi_trace_hits list what a BALL swept along each
 *                     ray touches, its radius the bits of rt_ray._reserved: see "sphere-cast-all" below.  Other values are refused with -2
 *                     and nothing changes.  Independent of "sweep"; every other call ignores it; at 0 the three calls are what they were
 *   "shade_threshold" k_stream: lanes (1..64) with a complete query that end a traversal burst (default 48)
 *   "node_min"        k_stream: inside a burst the node loop goes on while at least this many lanes hold an internal node (or no
 *                     lane holds a leaf); below it the leaves are served first (default 10; 1 = classic while-while)
 *   "tiles_per_fetch" k_stream: work items a wave reserves per fetch while the launch's queue is long (1..32, default 16 = the 16 sub-tiles of
 *                     one 8x8 tile); the units of the group — a pixel's sample chain (PCG) or one sub-stream of a pixel's samples (Philox) —
 *                     are handed to whichever lanes ask, in order, so nobody waits for the lane that drew the most expensive ones
 *   "fetch_guide", "fetch_guide_philox"   k_stream: guided self-scheduling — groups of tiles_per_fetch items while more than fetch_guide
 *                     groups per wave of the launch are left in the queue, then items_left / (waves x fetch_guide), down to single items
 *                     (default 4 for the PCG stream, 1 in Philox mode, whose units are small)
 *   "tile_sync"       k_stream: 1 = a wave takes a whole 8x8 tile at a time, 0 = lanes refill pixel by pixel
 *   "stream_tile"     k_stream: frames interleaved in a wave, as log2: 0 = 8x8 pixels of one frame, 2 = 4x4 pixels x 4 frames of the
 *                     launch, 4 = 2x2 pixels x 16 frames (default; launches shorter than the group fall back to 8x8 x 1)
 *   "device_bvh"      1 = build the BVH on the device (Morton order, PLOC clustering, sweep-SAH treelet passes, breadth-first collapse to
 *                     4-wide nodes: 100k triangles in 2.5 ms, 1M in 5.4 ms, traced within about 1 % / within -4 .. +2 % of the host tree), 0 = the
 *                     host's binned-SAH builder (50 ms / 600 ms), -1 (default) = device for rt_upload_local_meshes (meshes that move) and
 *                     for a world-space scene that is uploaded again within 16 traced frames of its last build (the reference's way of
 *                     animating: everything re-sent every frame), host for the first build of a world-space scene.  Triangles uploaded from
 *                     device memory ("device_geometry") are always built on the device, whatever this says: the host builder has no
 *                     positions to read
 *   "device_geometry" 0 (default) = rt_upload_triangles / rt_multi_upload_triangles read `tris` as host memory, as ever (no pointer query);
 *                     1 = `tris` may also lie in memory of the context's device (hipMalloc'ed or managed; the first context's for rt_multi).  The
 *                     call then copies n * 72 bytes device to device into the context's own buffer, on the context's stream (rt_set_stream),
 *                     at call time: the caller's writes to `tris` must be ordered before the call (the same stream, or synchronised), and the
 *                     caller may overwrite `tris` in work it orders after that stream.  No copy of the triangles is kept on the host.  A host
 *                     pointer takes the usual path.  Refused with -2, nothing changed: n < 0, a device pointer that is not 4-byte aligned,
 *                     memory of another device (n > 2^28: -3).  Such a scene is always built by the device builder.  An upload of the same
 *                     number of triangles over a tree built this way — no rt_upload_meshinfo, rt_upload_spheres or builder option since — is a
 *                     DEFORMATION: the next frame or query rewrites the tracer's triangle records in place (k_deform_update), refits the
 *                     boxes, and rebuilds on the device only under "rebuild_percent"'s rule (rt_stats.bvhRebuilds; lastGeometryMs is the
 *                     update's time).  Anything else is a new scene with a full device build.  rt_upload_meshinfo stays a host upload, and its
 *                     boundsMin / boundsMax stay the caller's, as in the reference: a caller who deforms keeps them current (a min / max over
 *                     the corners) or uses RT_INTERSECT_BRUTE.  Spheres, local meshes and transforms are host uploads
 *   "bvh_treelets"    device builder: number of sweep-SAH passes over the clustering's tree (default 6; 0 = none).  Pass k rebuilds, one wave
 *                     each, every maximal subtree of <= 64 * 8^k triangles over its subtrees of <= 8^k triangles (pass 0: over the triangles
 *                     themselves) with an exact sweep SAH — all three axes, every split position, large-box isolation — in the node slots the
 *                     subtree already has (csrc/rt_bvh_gpu.hpp step 3c).  "bvh_treelet_ratio" (8), "bvh_treelet_first" (1) and
 *                     "bvh_treelet_isolate" (1) tune the scale step, the first pass's item size and the isolation candidate
 *   "bvh_radius"      device builder: PLOC search radius; n > 0: n in the first rounds, doubled once a quarter and again once a sixteenth of
 *                     the clusters is left; n < 0: |n| in every round (default -16)
 *   "bvh_top"         device builder: n > 0 = once its bottom-up rounds have left at most n clusters, the top of the tree is built by the host's
 *                     binned-SAH split search over the clusters' boxes (round 3's way, default then 1024); 0 (default) = all on the device
 *   "peer_copies"     rt_multi: 1 = its device-to-device copies (scene fan-out, frame-end gather) go through hipMemcpyPeerAsync even between
 *                     contexts of one device — the branch a multi-GPU node takes, made runnable on a one-GPU box (default 0: peer API only
 *                     across devices)
 *   "rebuild_percent" on-device geometry pipeline: after a refit, rebuild on the device once the summed internal box area exceeds
 *                     this percentage of its value right after the last build (default 200; 0 = never)
 *   "compact_nodes"   k_trace / k_stream: 1 = traverse the f16 form of the BVH nodes (5 loads per node visit, default), 0 = the
 *                     f32 form (7 loads)
 *   "primary_lists"   k_stream, depth of field off: 1 (default) = every pixel's camera rays start from the <= 4 BVH leaves that can hold their
 *                     closest hit — found once per camera / scene (0.7 ms at 1080p) by tracing the corners of the pixel's jitter footprint
 *                     (csrc/rt_primary.hpp) — instead of from the root; 0 = always from the root.  The image does not depend on it.
 *   "queue_depth", "queue_linger_us"   rt_submit_frame: most frames the queue's worker puts into one launch (1..256, default 64); how long
 *                     it waits for more frames after the first one of an idle queue arrived (default 200 us: a burst becomes one launch)
 *   "blocks_per_cu"   cap on resident workgroups per CU (0 = occupancy query)                                     */
int rt_set_option(rt_ctx* ctx, const char* name, int value);

/* Row strip rendered by this context: rows [row0, row0+nrows) of the full width x height image.
 * Seeds use global pixel coordinates (RayTracing.shader:360-362) so the image is decomposition-invariant.
 * Default = the whole image.                                                                          */
int rt_set_rows(rt_ctx* ctx, int row0, int nrows);
/* Interleaved decomposition for load balance: this context renders the 8-row bands first_band, first_band +
 * band_stride, first_band + 2*band_stride, ... (band b = image rows [8b, 8b+8)); its targets hold those rows back to
 * back.  (0, 1) is the whole image.  Overrides rt_set_rows; rt_set_rows switches back to one contiguous strip.       */
int rt_set_bands(rt_ctx* ctx, int first_band, int band_stride);

/* One frame = Graphics.Blit(null, currentFrame, rayTracingMaterial) with "Frame" = frame_index, followed by
 * the Accumulate blit with "_Frame" = frame_index (RayTracingManager.cs:74-81).  Returns after the
 * stream has been synchronised.                                                                        */
int rt_render_frame(rt_ctx* ctx, int frame_index);
/* n_frames consecutive frames first_frame, first_frame+1, ... (one stream sync at the end).            */
int rt_render(rt_ctx* ctx, int first_frame, int n_frames);
/* As rt_render, but a counting build of the same kernel fills rt_stats' work counters.                 */
int rt_render_counting(rt_ctx* ctx, int first_frame, int n_frames);
/* Same frame computed by the reference's own flat loop (all spheres, all chunks, all triangles of
 * passing chunks) on the GPU — a validation/baseline path, not the fast path.                          */
int rt_render_frame_flat(rt_ctx* ctx, int frame_index);

/* Per-frame cameras (the reference reads the camera again on every OnRenderImage, RayTracingManager.cs:104,126-133, and keeps
 * accumulating).  The CAMERA FIELDS of rt_params are viewParams, camLocalToWorld and worldSpaceCameraPos; every other field is a
 * setting.  params holds n_frames entries: entry f is the uniforms of frame first_frame + f.  The result (resultTexture, the last
 * frame, numRenderedFrames and the context's params afterwards = params[n_frames - 1]) is bit for bit that of
 *     for f: rt_set_params(ctx, &params[f]); rt_render_frame(ctx, first_frame + f);
 * but the frames share launches: frames that differ in camera are traced by one k_stream launch with a camera table.  Every entry
 * must have the same settings (else -2, and nothing is rendered or changed); when they differ from the context's, the call first
 * acts as rt_set_params(&params[0]).  Byte-identical entries take rt_render's path.                                            */
int rt_render_params(rt_ctx* ctx, int first_frame, int n_frames, const rt_params* params);

/* Queued submission for a host that renders frame by frame, as the reference does (one trace blit + one accumulate blit per
 * OnRenderImage, RayTracingManager.cs:74-91).  rt_submit_frame returns at once; a worker thread of the library traces what has queued
 * up while the previous launch ran — consecutive frame indices share ONE launch (frame-interleaved work items, one launch tail: the
 * batched rate instead of the single-frame rate) — and accumulates in submission order, so the image equals rt_render's over the same
 * frames bit for bit.  rt_wait returns when everything submitted is in resultTexture; every other call on the context waits first, so
 * reading, changing the camera or uploading between submissions is always safe.  An error of a queued launch is reported (once) by
 * the next call that waits.  Option "queue_depth": most frames per launch (default 64).                                        */
int rt_submit_frame(rt_ctx* ctx, int frame_index);
int rt_wait(rt_ctx* ctx);
/* rt_submit_frame with the frame's own uniforms (*params is copied).  A frame whose params differ from those in effect at the tail of
 * the queue only in the camera fields (see rt_render_params) is queued without waiting and may share a launch with its neighbours; a
 * change of settings waits for the queue, applies the new params as rt_set_params does, then queues the frame.  Errors as for
 * rt_submit_frame.  rt_submit_frame queues a frame with the params in effect at the tail of the queue.                       */
int rt_submit_frame_params(rt_ctx* ctx, int frame_index, const rt_params* params);

/* Zero the accumulation target and the frame counter (RayTracingManager.Start, :43-46).                */
int rt_reset_accum(rt_ctx* ctx);

/* Read back RGBA32F rows of this context's strip (nrows*width*4 floats).  accum = resultTexture,
 * last_frame = currentFrame (RayTracingManager.cs:33,75).                                             */
int rt_read_accum     (rt_ctx* ctx, float* rgba, size_t n_floats);
int rt_read_last_frame(rt_ctx* ctx, float* rgba, size_t n_floats);
/* Restore a saved accumulation state: resultTexture + numRenderedFrames are all the reference carries from frame to frame
 * (RayTracingManager.cs:26,33; the counter restarts in Start, :43-46).  rgba = rows*width*4 floats as returned by
 * rt_read_accum; the next frame to render is frame index frames_rendered (frames are independent given their index,
 * RayTracing.shader:362, so a resumed render equals an uninterrupted one bit for bit).                                  */
int rt_write_accum(rt_ctx* ctx, const float* rgba, size_t n_floats, int frames_rendered);
/* Device-side copy of the strip into caller-owned device memory (e.g. a torch tensor handed to RCCL). */
int rt_copy_accum_to_device(rt_ctx* ctx, void* dst_device_ptr, size_t n_floats);

/* Display step after the path: resultTexture converted linear -> sRGB, 8 bits per channel (R | G<<8 | B<<16 | A<<24),
 * as the final Blit(resultTexture, target) into the sRGB back buffer does (RayTracingManager.cs:84;
 * ProjectSettings.asset:50).  n_pixels = rows*width of this context's strip; row 0 is the bottom row.             */
int rt_read_display(rt_ctx* ctx, uint32_t* rgba8, size_t n_pixels);

int rt_get_stats(rt_ctx* ctx, rt_stats* out);

/* Diagnostics: the acceleration structure the library built behind the reference's flat chunk list (the reference has none:
 * RayTracing.shader:276-294 loops over all chunks) — n_nodes = rt_stats.numBvhNodes records of 128 bytes each, in the f32
 * form (six plane arrays of 4 floats, child[4], meta[4]) and in the f16 form the kernels traverse (csrc/bvh.hpp Node4h).
 * Either destination may be NULL.  Tests check that every f16 box contains its f32 box.                                 */
int rt_read_bvh(rt_ctx* ctx, void* nodes_f32, void* nodes_f16, size_t n_nodes);
/* Diagnostics: the triangle order the leaf references of rt_read_bvh point into — order[i] = the uploaded triangle at BVH
 * position i (rt_upload_triangles order for world-space uploads, rt_read_world_geometry order for local meshes: the `primitive`
 * numbering of rt_hit).  n = the triangles in the tree (the sum of the leaf counts): every uploaded triangle after a device
 * build, those a chunk addresses after a host build; 0 is legal.  Tests audit every box of every tree against its triangles.  */
int rt_read_bvh_order(rt_ctx* ctx, uint32_t* order, size_t n);

/* ---- ray queries: what a caller-supplied ray hits -------------------------------------------------------------------
 * The reference answers "what does this ray hit?" only inside its shader: CalculateRayCollision (RayTracing.shader:256-297) over
 * every sphere, then every chunk whose RayBoundingBox passes (:276-294), strict '<' throughout.  These calls run that function for
 * rays the caller makes (picking, autofocus, line of sight) against the scene the next frame would trace, through the library's
 * BVH; the answer is the reference's bit for bit in every field of rt_hit.
 *
 *   closest hit   hits[i] = CalculateRayCollision(origin, direction) when its dst < tMax, else a miss.  The context's
 *                 intersectMode applies (RT_INTERSECT_FLAT_CHUNKS when rt_set_params was never called: a query needs no params).
 *   occlusion     occluded[i] = 1 exactly when the closest-hit query with the same ray hits: an any-hit traversal that stops at the
 *                 first sphere or triangle with dst < tMax (in FLAT_CHUNKS mode, one whose chunk's box test passes).
 *   scene         the queue is settled first; then the scene is made current as for a frame (pending uploads, moved meshes).  The box
 *                 padding is widened, as for a camera, when the largest finite |origin coordinate| of the rays that are traced exceeds
 *                 what the boxes were padded for (rt_stats.bvhRepads; local uploads: one geometry pass).  Nothing else changes: no
 *                 accumulation state, frame counter or work counter moves (only bvhBuilds / bvhRebuilds / bvhRepads, when the query
 *                 triggered that build or re-padding).  The widened padding outlives the query, as a camera's does: boxes padded for
 *                 origins far out prune less, so later frames trace slower until the next build (a new upload).
 *   arguments     n == 0 returns 0; a null context -1; n < 0, a null buffer with n > 0, or a device pointer of another device
 *                 (device entries: also one not 16-byte aligned) -2 with a message in rt_last_error.                              */
typedef struct rt_ray {                 /* 32 B */
    float   origin[3];
    float   tMax;                       /* only hits with dst < tMax count; +inf = unbounded; <= 0 or NaN = a miss, nothing is traced */
    float   direction[3];               /* not normalised by the library: dst is in units of |direction|, as in the shader             */
    int32_t _reserved;                  /* option "sweep" = 1: the bits of the ball's radius, a float; never read otherwise            */
} rt_ray;

enum { RT_HIT_NONE = 0, RT_HIT_SPHERE = 1, RT_HIT_TRIANGLE = 2 };

typedef struct rt_hit {                 /* 64 B; a miss: dst = +inf, hitPoint = normal = 0, kind = RT_HIT_NONE, indices -1, u = v = 0 */
    float   dst;                        /* CalculateRayCollision's closest.dst (:256-297)                                               */
    float   hitPoint[3];                /* origin + direction * dst (RaySphere :141, RayTriangle :170)                                  */
    float   normal[3];                  /* the shading normal Trace uses: sphere normalize(hitPoint - centre) (:142), triangle the       */
                                        /* normalised interpolation of the vertex normals (:171)                                        */
    int32_t kind;                       /* RT_HIT_*                                                                                      */
    int32_t primitive;                  /* sphere: index in the uploaded sphere buffer; triangle: index in the world triangle buffer     */
                                        /* (rt_upload_triangles order; local uploads: rt_read_world_geometry order); else -1             */
    int32_t chunk;                      /* triangle: its rt_meshinfo index (the chunk whose material shades it); else -1                 */
    int32_t mesh;                       /* triangle of an rt_upload_local_meshes scene: its mesh index; else -1                          */
    float   u, v;                       /* triangle: RayTriangle's u, v (:163-165; w = 1 - u - v); else 0                                */
    int32_t _reserved[3];               /* 0; option "sweep" = 1: [0] = the contact's feature code                                       */
} rt_hit;

/* Host memory; return when the results are in hits / occluded.  The rays go through device buffers of the context in slices of at
 * most 4M rays, so the memory used does not grow with n.                                                                        */
int rt_trace_rays (rt_ctx* ctx, const rt_ray* rays, int n, rt_hit* hits);
int rt_occluded   (rt_ctx* ctx, const rt_ray* rays, int n, uint8_t* occluded);
/* Device memory of the context's GPU (rays: n rt_ray, hits: n rt_hit, occluded: n bytes; rays and hits 16-byte aligned), ordered on
 * the context's stream (rt_set_stream; switching the stream away afterwards keeps the order: the next stream waits for the query).  The call returns once the query is enqueued, with one exception to the asynchrony: the
 * box padding needs the largest |origin coordinate| of the batch, so a small reduction kernel runs first and the call waits for
 * its 4-byte result (a stream synchronisation) before it enqueues the query.                                                     */
int rt_trace_rays_device(rt_ctx* ctx, const void* rays, int n, void* hits);
int rt_occluded_device  (rt_ctx* ctx, const void* rays, int n, void* occluded);

/* ---- sphere casts: how far a ball travels along a caller-supplied ray before it touches something --------------------------------
 * Option "sweep" = 1 (rt_set_option) turns the six ray-query calls above into Unity's Physics.SphereCast / CheckSphere along a path:
 * character controllers, camera collision, line of sight with clearance, thick projectiles, probe placement.  No new entry: the rays,
 * the records, the slicing (the result never depends on it), the origin-bound reduction and padding rule, the stream ordering, the
 * error rules and "nothing else moves" are the ray queries'.  The reference has no such function; the definition is this library's own
 * and frozen to the bit: float32, every product and sum rounded on its own (no FMA), / and sqrtf IEEE, dot and cross as in
 * "closest-point queries" below.  The answer is the same bits whatever the tree, the builder, the leaf size or the order of the visit.
 *
 *   input         origin o, direction d (not normalised: dst is in units of |d|) and tMax as for a ray; r = the float whose bits are
 *                 _reserved.  Not traced — the miss record, occluded 0 — when tMax <= 0 or NaN, or r <= 0, NaN or infinite.
 *   candidates    every uploaded sphere, and every triangle of the tree: the ones rt_read_bvh_order lists, as for closest-point
 *                 queries.  intersectMode plays no part (no chunk box is tested) and no rt_params are needed.
 *   scene sphere  (centre s, radius R)  RaySphere (RayTracing.shader:120-146) with the radius R + r: oc = o - s; a = dot(d, d);
 *                 b = 2 * dot(oc, d); c = dot(oc, oc) - (R + r) * (R + r); disc = b * b - 4 * a * c; t = (-b - sqrtf(disc)) / (2 * a),
 *                 accepted when disc >= 0 and t >= 0 — so a ball that starts overlapping a sphere does not report that sphere, as a ray
 *                 that starts inside does not.  centre = o + d * t; normal = normalize(centre - s); hitPoint = centre - normal * r.
 *                 Feature code 0.
 *   triangle      A = posA, eAB = posB - posA, eAC = posC - posA, n = cross(eAB, eAC) (the floats RayTriangle forms), B = A + eAB,
 *                 C = A + eAC.  Two-sided, seven features, in this order:
 *                   faces     N = n * (1 / sqrtf(dot(n, n))).  Front (code 1): the two-sided RayTriangle of the multi-hit queries from the
 *                             origin o - N * r, accepted when it reports the front face (det >= 1e-6f).  Back (code 2): from o + N * r,
 *                             the back face (det <= -1e-6f).  t, u, v are that test's; hitPoint = the moved origin + d * t.
 *                   edges     AB (code 3: P = A, e = eAB), AC (4: P = A, e = eAC), BC (5: P = B, e = eAC - eAB): m = o - P;
 *                             ee = dot(e, e); md = dot(m, e); nd = dot(d, e); dd = dot(d, d); qa = ee * dd - nd * nd;
 *                             qb = ee * dot(m, d) - nd * md; qc = ee * (dot(m, m) - r * r) - md * md; disc = qb * qb - qa * qc;
 *                             accepted when qa > 0 && disc >= 0, t = (-qb - sqrtf(disc)) / qa >= 0, and s = md + t * nd has 0 < s < ee.
 *                             q = s / ee; hitPoint = P + e * q; (u, v) = (q, 0), (0, q), (1 - q, q).
 *                   vertices  A, B, C (codes 6, 7, 8): RaySphere with the vertex as centre and radius r.  hitPoint = the vertex;
 *                             (u, v) = (0, 0), (1, 0), (0, 1).
 *   guard         a triangle feature's candidate counts only if the ball at its time really touches the triangle: with
 *                 c = o + d * t, the key k of the closest-point query of c against this triangle (below) must satisfy k <= g * g,
 *                 g = r * (1 + 2^-6), both products floats.  (An edge's quadratic cancels badly when d is nearly parallel to e; a t
 *                 that is wrong by more than the guard allows is refused rather than reported, and it is the guard that makes the
 *                 answer independent of the tree: the BVH's boxes are moved outwards by at least g plus their padding, so no candidate
 *                 that counts lies in a node that is skipped.)  A scene sphere has no guard.
 *   answer        among the candidates with t < tMax (strict) the smallest (t, kind, primitive, feature code): at equal t a sphere
 *                 before a triangle, then the lower uploaded index, then the lower code.  dst = t; hitPoint as above; for a triangle
 *                 normal = normalize((o + d * t) - hitPoint).  normal is the CONTACT normal — from the contact point to the ball's
 *                 centre — not rt_hit's shading normal: no vertex normal is read.  kind, primitive, chunk, mesh, u, v as in rt_hit;
 *                 _reserved[0] = the feature code, _reserved[1..2] = 0.  occluded[i] = 1 exactly when this answer is a hit.
 *   limits        float32 limits the balls that are found.  A quadratic's root puts the ball about 2^-25 * (|o - P| / r)^2 * r off the
 *                 feature at the computed time, P the feature: within the guard's 2^-6 * r up to about 700 radii away — there the
 *                 first contact is found, a float64 evaluation names the same feature, and a ball that started free is within 2 % of r
 *                 of every surface.  From thousands of radii away contacts are reported late, through a neighbouring feature, or not at
 *                 all, and a scene sphere's root is RaySphere's, off by whole radii at 1e4 scene extents: a caller that far away advances
 *                 the origin along d first and adds the advance to dst.  A ball smaller than the float spacing of the coordinates finds
 *                 little.  None of this is repaired: the definition is what tests/sweep_oracle.c restates, bit for bit.  r * r or g * g
 *                 beyond float range: whatever the arithmetic gives (the tree then prunes nothing).                                  */

/* ---- radiance queries: how much light arrives along a caller-supplied ray ---------------------------------------------
 * Between "what image does the camera see?" (the frame calls) and "what does this ray hit?" (the ray queries): Trace
 * (RayTracing.shader:300-352) for rays the caller makes — light probes, lightmap texels, a reflection probe, a fisheye or stereo camera,
 * the radiance behind a picked pixel.  For ray i of a call, with o its origin, d its direction (not normalised by the library: Trace
 * runs on it as given, so a caller who wants the shader's behaviour passes unit directions), t its tMax and K = firstIndex + i:
 *
 *   settings      the context's current rt_params (without any the call fails): maxBounceCount, intersectMode, environmentEnabled, the
 *                 sky fields and worldSpaceLightPos0 apply; the camera fields, numRaysPerPixel and rngMode do not.  The stream is always
 *                 the Philox one, as for the feature buffers.
 *   sample s      (0 <= s < N = samples) Trace(o, d) exactly as RT_RNG_PHILOX defines it, with key (K, seed) and counter (block, s, 0,
 *                 0): the hit at loop index b draws from blocks 1 + 2b and 2 + 2b.  Block 0, a frame's camera ray, is unused: the caller
 *                 made the ray.  One change: the cast at loop index 0 counts only hits with dst < t (rt_trace_rays' rule:
 *                 CalculateRayCollision, then the comparison).  The cast after an InvisibleLight pass-through and every later cast is
 *                 unbounded, as in the shader.
 *   sum           the fixed tree of the Philox mode: S = 16 / 4 / 1 sub-streams for N >= 16 / >= 4 / else, sample s in sub-stream s mod
 *                 S, each sub-stream added in increasing order from 0.0f, the S sub-sums added pairwise ((k, k + 1), then (k, k + 2),
 *                 ...), the root divided by (float)N per channel: rgba[i] = (r, g, b, 1.0f).
 *   not traced    t <= 0 or NaN: rgba[i] = (0, 0, 0, 0), no cast.
 *   defaults      params == NULL: samples = the context's numRaysPerPixel, seed 0, firstIndex 0.
 *   non-finite    ray components that are not finite give whatever this arithmetic gives; the call does not fault and a path ends
 *                 after maxBounceCount + 1 casts.
 *   scene, state  as for ray queries: the queue is settled, the scene made current, the box padding widened for the batch's largest
 *                 finite |origin coordinate| among rays with t > 0 (the device entry measures it with the ray queries' reduction kernel
 *                 and the same single synchronisation).  Nothing of the image path, the feature planes, the denoiser or the temporal
 *                 state moves, and no rt_stats field except bvhBuilds / bvhRebuilds / bvhRepads when the call triggered them.
 *   splitting     a batch split anywhere into two calls, the second with firstIndex advanced by the first's length, gives the bits of
 *                 one call: the library's own slices (option "radiance_slice", rays per launch) and rt_multi are invisible.
 *   errors        a null handle -1; n == 0 returns 0; no params set, n < 0, a null buffer with n > 0, samples outside 1..65536, a
 *                 non-zero reserved word, and for the device entry a pointer of another device or one not 16-byte aligned: -2 with a
 *                 message, and nothing changes.                                                                                   */
typedef struct rt_radiance_params {     /* 32 B */
    int32_t  samples;                   /* N, 1..65536: independent runs of Trace per ray                                    */
    uint32_t seed;                      /* second key word of the Philox stream (what Frame is for a frame)                  */
    uint32_t firstIndex;                /* ray i of the call has stream index firstIndex + i (wraps mod 2^32)                */
    int32_t  _reserved[5];              /* must be 0                                                                         */
} rt_radiance_params;
typedef struct rt_radiance_info {       /* 32 B */
    int32_t samples;                    /* of the last call                                                                  */
    int32_t lastSampleLanes;            /* lanes of a wave that shared a ray's samples in the last launch: 16, 4 or 1        */
    int32_t calls, _reserved;
    double  lastKernelMs, totalKernelMs;   /* HIP-event time of the launches of the last host-entry call / summed            */
} rt_radiance_info;
/* Host memory (rgba: n * 4 floats); returns when the results are in rgba.  Slices as for rt_trace_rays.                            */
int rt_trace_radiance       (rt_ctx* ctx, const rt_ray* rays, int n, const rt_radiance_params* params, float* rgba);
/* Device memory of the context's GPU (rays: n rt_ray, rgba: n float4, both 16-byte aligned), ordered on the context's stream as
 * rt_trace_rays_device is; rt_radiance_info counts the call and keeps the host entry's times.                                     */
int rt_trace_radiance_device(rt_ctx* ctx, const void* rays, int n, const rt_radiance_params* params, void* rgba);
int rt_get_radiance_info    (rt_ctx* ctx, rt_radiance_info* out);

/* ---- gather queries: the light that arrives at a point, over a hemisphere or the sphere ------------------------------------
 * What a lightmap texel, an irradiance probe or an SH light probe asks.  A radiance query averages N runs of Trace along ONE direction;
 * here the library draws a direction per sample on the device, from the same counter-based stream, and sums in the wave: n points go
 * up, n (or 9 n) float4 come back.  A point is an rt_ray: origin is the position, direction is the NORMAL n (used as given: pass a unit
 * normal, or zero), tMax bounds the first cast.  For point i of a call, K = firstIndex + i, and sample s (0 <= s < N = samples):
 *
 *   direction     R = RandomDirection as the shader defines it (RayTracing.shader:216-223: six draws, the shader's order) from the
 *                 Philox stream with key (K, seed) and counter (block, s, 0, 0): words 0..3 of block 0xFFFFFFFE, then words 0, 1 of
 *                 block 0xFFFFFFFF.  Trace's hits use blocks 1 + 2b and 2 + 2b with b <= 32000, so the two never meet; block 0 stays
 *                 unused, as for radiance queries.
 *                 RT_GATHER_COSINE (mode 0): d = normalize(n + R), the diffuse lobe of :328 — cosine-distributed about a unit n,
 *                 uniform over the sphere when n = 0.  RT_GATHER_SH9 (mode 1): d = R; n is ignored.
 *   sample        L_s = Trace(origin, d) exactly as a radiance query runs it for key (K, seed) and sample s: the cast at loop index 0
 *                 counts only hits with dst < tMax, every later cast is unbounded, the context's rt_params apply as they do there.
 *                 origin is used as given — the library adds NO offset: a caller on a surface moves the point off it along n
 *                 themselves (the tests use 1e-3 * n).
 *   sum           the fixed tree of the Philox mode over the N samples, per channel (S = 16 / 4 / 1 sub-streams for N >= 16 / >= 4 /
 *                 else, sample s in sub-stream s mod S, each added in increasing order from 0.0f, then pairwise (k, k + 1), (k, k + 2),
 *                 ...).
 *   mode 0 output one float4 per point: (root.rgb / (float)N, 1.0f) — the MEAN RADIANCE over the lobe.  For a unit n the irradiance
 *                 is pi times it (the cosine-weighted integral with the lobe's pdf cos / pi).
 *   mode 1 output nine float4 per point (144 B), coefficient k = 0..8 of the real SH basis, bands 0..2.  With d = (x, y, z) the
 *                 per-sample term is L_s.c * Y_k for each channel c; in float32, every product a separate rounding, no FMA:
 *                   Y0 = 0.28209479f            Y1 = 0.48860251f*y          Y2 = 0.48860251f*z         Y3 = 0.48860251f*x
 *                   Y4 = 1.09254843f*(x*y)      Y5 = 1.09254843f*(y*z)      Y6 = 0.31539157f*(3.0f*(z*z) - 1.0f)
 *                   Y7 = 1.09254843f*(x*z)      Y8 = 0.54627421f*(x*x - y*y)
 *                 The 27 channels go through the same tree; out[k] = ((root / (float)N) * 12.566371f, w), dividing first, with
 *                 w = 1.0f for k = 0 and 0.0f otherwise: the projection of the incoming radiance (uniform pdf 1 / (4 pi)).
 *   not traced    tMax <= 0 or NaN: every output float of the point is 0; no draw, no cast.
 *   defaults      params == NULL: samples = the context's numRaysPerPixel, seed 0, firstIndex 0, mode 0.
 *   non-finite    components that are not finite give whatever this arithmetic gives; the call does not fault and a path ends after
 *                 maxBounceCount + 1 casts.
 *   scene, state  as for radiance queries: the queue is settled, the scene made current, the box padding widened for the largest finite
 *                 |origin coordinate| among points with tMax > 0.  Nothing of the image, feature, denoiser, temporal or radiance state
 *                 moves, and no rt_stats field except bvhBuilds / bvhRebuilds / bvhRepads.
 *   splitting     a batch cut anywhere into two calls, the second with firstIndex advanced by the first's length, gives the bits of one
 *                 call: the library's own slices (option "gather_slice", points per launch) and rt_multi are invisible.
 *   errors        a null handle -1; n == 0 returns 0; no params set, n < 0, a null buffer with n > 0, samples outside 1..65536, a
 *                 non-zero reserved word, a mode that is not 0 or 1, and for the device entry a pointer of another device or one not
 *                 16-byte aligned: -2 with a message, and nothing changes.                                                        */
enum { RT_GATHER_COSINE = 0, RT_GATHER_SH9 = 1 };
typedef struct rt_gather_params {       /* 32 B */
    int32_t  samples;                   /* N, 1..65536: directions per point                                                 */
    uint32_t seed;                      /* second key word of the Philox stream                                              */
    uint32_t firstIndex;                /* point i of the call has stream index firstIndex + i (wraps mod 2^32)              */
    int32_t  mode;                      /* RT_GATHER_*                                                                       */
    int32_t  _reserved[4];              /* must be 0                                                                         */
} rt_gather_params;
typedef struct rt_gather_info {         /* 32 B */
    int32_t samples;                    /* of the last call                                                                  */
    int32_t lastSampleLanes;            /* lanes of a wave that shared a point's samples in the last launch: 16, 4 or 1      */
    int32_t calls, mode;                /* calls so far / the last call's mode                                               */
    double  lastKernelMs, totalKernelMs;   /* HIP-event time of the launches of the last host-entry call / summed            */
} rt_gather_info;
/* Host memory (out: n * 4 floats in mode 0, n * 36 in mode 1); returns when the results are in out.  The points go through device
 * buffers of the context in slices of "gather_slice" points, sized to min(n, slice).                                              */
int rt_gather        (rt_ctx* ctx, const rt_ray* points, int n, const rt_gather_params* params, float* out);
/* Device memory of the context's GPU (points: n rt_ray, out: n or 9 n float4, both 16-byte aligned), ordered on the context's stream
 * as rt_trace_rays_device is; rt_gather_info counts the call and keeps the host entry's times.                                     */
int rt_gather_device (rt_ctx* ctx, const void* points, int n, const rt_gather_params* params, void* out);
int rt_get_gather_info(rt_ctx* ctx, rt_gather_info* out);

/* ---- visibility gathers: how open a point is, in which direction, and how far away the surfaces are ------------------------------
 * The geometry-only question beside a gather query: ambient occlusion and bent normals of a lightmap texel or vertex, the sky
 * visibility and a visibility SH9 of a probe (to multiply with a sky SH9), the mean distance and mean squared distance that place
 * probes and detect probes inside walls.  Nothing is shaded and no rt_params are needed.  A point is an rt_ray as for rt_gather: origin
 * is the position, direction is the NORMAL n (used as given: pass a unit normal, or zero), tMax is the REACH t of every cast.  For point
 * i of a call, K = firstIndex + i, and sample s (0 <= s < N = samples):
 *
 *   direction     R = RandomDirection exactly as rt_gather draws it: the Philox stream with key (K, seed) and counter (block, s, 0, 0),
 *                 words 0..3 of block 0xFFFFFFFE, then words 0, 1 of block 0xFFFFFFFF.
 *                 RT_VIS_COSINE (mode 0) and RT_VIS_DISTANCE (mode 2): d = normalize(n + R) — cosine-distributed about a unit n,
 *                 uniform over the sphere when n = 0.  RT_VIS_SH9 (mode 1): d = R; n is ignored.  For equal (K, seed, s, n) these are
 *                 the bits rt_gather's modes 0 / 1 trace along: one set of directions serves a probe's lighting and its visibility.
 *   cast, 0 and 1 occ = what rt_occluded answers for the ray (origin, d, t): the any-hit rule with dst < t.  The context's intersectMode
 *                 applies (RT_INTERSECT_FLAT_CHUNKS when rt_set_params was never called).  v = occ ? 0.0f : 1.0f.
 *   cast, mode 2  h = what rt_trace_rays answers for (origin, d, t); r = h is a hit ? h.dst : t; hit = 1.0f for a hit, 0.0f for a miss.
 *   channels      (a select, so that 0 x NaN cannot appear)
 *                 mode 0, four:  (v ? d.x : 0, v ? d.y : 0, v ? d.z : 0, v)
 *                 mode 1, ten:   v ? Y_k(d) : 0 for k = 0..8, then v; Y_k as the gather section writes it, every product a separate
 *                                rounding, no FMA
 *                 mode 2, three: (r, r * r, hit)
 *   sum           the fixed tree of the Philox mode over the N samples, per channel, as in rt_gather (S = 16 / 4 / 1 sub-streams for
 *                 N >= 16 / >= 4 / else, sample s in sub-stream s mod S, each added in increasing order from 0.0f, then pairwise); the
 *                 root is divided by (float)N.
 *   mode 0 output one float4 per point: (bent.xyz, visibility).  bent is the mean open direction, NOT normalised: its length tells how
 *                 one-sided the opening is.  Ambient occlusion = 1 - visibility.
 *   mode 1 output three float4 per point (48 B): floats 0..8 = (root_k / (float)N) * 12.566371f, dividing first — the projection of the
 *                 visibility function onto the real SH basis of bands 0..2; float 9 = the visibility fraction; floats 10, 11 = 0.0f.
 *   mode 2 output one float4 per point: (mean r, mean r * r, hit fraction, 1.0f).  With an infinite t a miss makes both means +inf.
 *                 The 0 / 1 channels sum exactly up to 2^24, so visibility and hit fraction equal count / (float)N whatever the tree.
 *   not traced    t <= 0 or NaN: every output float of the point is 0; no draw, no cast.
 *   non-finite    components that are not finite, or n + R = 0, give whatever this arithmetic gives; the call does not fault.
 *   scene, state  as for ray queries: the queue is settled, the scene made current, the box padding widened for the largest finite
 *                 |origin coordinate| among points with t > 0.  Nothing else moves — not the image, feature, denoiser, temporal,
 *                 radiance or gather state, and no rt_stats field except bvhBuilds / bvhRebuilds / bvhRepads.
 *   splitting     a batch cut anywhere into two calls, the second with firstIndex advanced by the first's length, gives the bits of one
 *                 call: the library's own slices (option "visibility_slice", points per launch) and rt_multi are invisible.
 *   defaults      params == NULL: samples = RT_VISIBILITY_DEFAULT_SAMPLES (64), seed 0, firstIndex 0, mode 0.
 *   errors        a null handle -1; n == 0 returns 0; n < 0, a null buffer with n > 0, samples outside 1..65536, a non-zero reserved
 *                 word, a mode outside 0..2, and for the device entry a pointer of another device or one not 16-byte aligned: -2 with
 *                 a message, and nothing changes.                                                                                  */
enum { RT_VIS_COSINE = 0, RT_VIS_SH9 = 1, RT_VIS_DISTANCE = 2 };
#define RT_VISIBILITY_DEFAULT_SAMPLES 64
typedef struct rt_visibility_params {   /* 32 B */
    int32_t  samples;                   /* N, 1..65536: directions per point                                                 */
    uint32_t seed;                      /* second key word of the Philox stream                                              */
    uint32_t firstIndex;                /* point i of the call has stream index firstIndex + i (wraps mod 2^32)              */
    int32_t  mode;                      /* RT_VIS_*                                                                          */
    int32_t  _reserved[4];              /* must be 0                                                                         */
} rt_visibility_params;
typedef struct rt_visibility_info {     /* 32 B */
    int32_t samples;                    /* of the last call                                                                  */
    int32_t lastSampleLanes;            /* lanes of a wave that shared a point's samples in the last launch: 16, 4 or 1      */
    int32_t calls, mode;                /* calls so far / the last call's mode                                               */
    double  lastKernelMs, totalKernelMs;   /* HIP-event time of the launches of the last host-entry call / summed            */
} rt_visibility_info;
/* Host memory (out: n * 4 floats in modes 0 and 2, n * 12 in mode 1); returns when the results are in out.  The points go through
 * device buffers of the context in slices of "visibility_slice" points, sized to min(n, slice).                                   */
int rt_visibility        (rt_ctx* ctx, const rt_ray* points, int n, const rt_visibility_params* params, float* out);
/* Device memory of the context's GPU (points: n rt_ray, out: n or 3 n float4, both 16-byte aligned), ordered on the context's stream
 * as rt_trace_rays_device is; rt_visibility_info counts the call and keeps the host entry's times.                                */
int rt_visibility_device (rt_ctx* ctx, const void* points, int n, const rt_visibility_params* params, void* out);
int rt_get_visibility_info(rt_ctx* ctx, rt_visibility_info* out);

/* ---- closest-point queries: the nearest surface to a point, its distance, and the side the point lies on ------------------------------
 * The one question of this group that is about a POINT, not a ray: which sphere or triangle is nearest to p, where on it, how far, and
 * on which side.  Signed-distance baking, pushing a probe out of a wall, snapping a picked position to geometry, proximity tests, the
 * offset a gather point needs.  The reference has no such function; the definition below is this library's own, in float32 with every
 * product and sum rounded on its own (no FMA), and the answer is the same bits whatever the tree, the builder, the leaf size or the
 * order of the visit.  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; cross, +, -, * on vectors are component-wise as in the shader;
 * / and sqrtf are IEEE.
 *
 *   input         an rt_ray: origin = the point p, tMax = the search radius R (+inf: unbounded).  direction and the reserved word are
 *                 never read.
 *   candidates    every uploaded sphere, and every triangle of the tree: the ones rt_read_bvh_order lists, those a ray query can hit.
 *                 intersectMode plays no part and no rt_params are needed.
 *   sphere        m = p - c; len = sqrtf(dot(m, m)); ds = fabsf(len - r); key k = ds * ds; dst = ds; point = c + m * (r / len);
 *                 side = len >= r ? +1 : -1; normal = normalize(point - c).  p on the centre: whatever this arithmetic gives.
 *   triangle      A = posA, eAB = posB - posA, eAC = posC - posA (the floats RayTriangle forms), ap = p - A.  The seven-region test
 *                 (Ericson, Real-Time Collision Detection 5.1.5) on these alone:
 *                   d1 = dot(eAB, ap); d2 = dot(eAC, ap); bp = ap - eAB; d3 = dot(eAB, bp); d4 = dot(eAC, bp);
 *                   cp = ap - eAC; d5 = dot(eAB, cp); d6 = dot(eAC, cp);
 *                   vc = d1 * d4 - d3 * d2; vb = d5 * d2 - d1 * d6; va = d3 * d6 - d5 * d4; d43 = d4 - d3; d56 = d5 - d6;
 *                 the first of these that holds decides (u, v):
 *                   d1 <= 0 && d2 <= 0                      vertex A   u = 0, v = 0
 *                   d3 >= 0 && d4 <= d3                     vertex B   u = 1, v = 0
 *                   vc <= 0 && d1 >= 0 && d3 <= 0           edge AB    u = d1 / (d1 - d3), v = 0
 *                   d6 >= 0 && d5 <= d6                     vertex C   u = 0, v = 1
 *                   vb <= 0 && d2 >= 0 && d6 <= 0           edge AC    u = 0, v = d2 / (d2 - d6)
 *                   va <= 0 && d43 >= 0 && d56 >= 0         edge BC    v = d43 / (d43 + d56), u = 1 - v
 *                   otherwise                               interior   den = (va + vb) + vc; u = vb / den; v = vc / den; then
 *                                                                      u = u < 0 ? 0 : u; u = u > 1 ? 1 : u; v = v < 0 ? 0 : v;
 *                                                                      v = v > 1 - u ? 1 - u : v   (rounding in va, vb, vc can leave the
 *                                                                      quotients just outside the triangle; a NaN stays a NaN)
 *                 q = (A + eAB * u) + eAC * v; e = p - q; key k = dot(e, e); dst = sqrtf(k); point = q;
 *                 s = dot(e, cross(eAB, eAC)); side = s > 0 ? +1 : s < 0 ? -1 : 0 (0 also for NaN); normal = rt_hit's: the normalised
 *                 interpolation of the vertex normals at (u, v).  A degenerate triangle falls into a vertex or edge region; if it
 *                 reaches the interior its denominator is 0 and the NaN key never wins.
 *   acceptance    a candidate counts when k < R * R (the product a float, the comparison strict; a NaN k never counts).  The winner is
 *                 the smallest (k, kind, primitive): at equal k a sphere comes before a triangle, then the lower uploaded index wins.
 *                 Ties are the normal case for a point over a shared edge or vertex.
 *   not searched  R <= 0 or NaN: the miss record, nothing is read.  A point with a NaN or infinite component has no candidate (every
 *                 key it forms is +inf or NaN): the miss record.
 *   side          +1 in front of a triangle (the side its winding's normal cross(eAB, eAC) points to) or outside a sphere, -1 behind /
 *                 inside.  As the sign of a distance field it is reliable for closed, consistently wound meshes away from creases: where
 *                 the closest point lies on an edge or vertex the sign is that of ONE of the faces that meet there (the lowest index), which
 *                 at a sharp crease can differ from the inside / outside of the solid.
 *   scene, state  as for ray queries: the queue is settled, the scene made current, the box padding widened for the largest finite
 *                 |coordinate| among points with R > 0.  Nothing else moves — not the image, feature, filter or other query state, and no
 *                 rt_stats field except bvhBuilds / bvhRebuilds / bvhRepads.  The library's slices ("closest_slice") and rt_multi are
 *                 invisible; a batch cut anywhere into two calls gives the bits of one.
 *   errors        a null handle -1; n == 0 returns 0; n < 0, a null buffer with n > 0, and for the device entry a pointer of another
 *                 device or one not 16-byte aligned: -2 with a message, and nothing changes.                                         */
typedef struct rt_closest {             /* 64 B; nothing within reach: dst = +inf, point = normal = 0, kind = RT_HIT_NONE, indices -1, u = v = 0, side = 0 */
    float   dst;                        /* unsigned distance from the query point to `point`                                            */
    float   point[3];                   /* the closest point of the closest primitive                                                   */
    float   normal[3];                  /* the shading normal there, as rt_hit.normal defines it                                        */
    int32_t kind;                       /* RT_HIT_*                                                                                     */
    int32_t primitive;                  /* exactly as in rt_hit                                                                         */
    int32_t chunk;
    int32_t mesh;
    float   u, v;                       /* triangle: point = A + (B - A) * u + (C - A) * v, rt_hit's convention; else 0                 */
    int32_t side;                       /* +1 / -1 / 0, see above                                                                       */
    int32_t _reserved[2];               /* 0; "closest_k" > 1 or "closest_all" = 1: [0] = the point's count (K-nearest queries), [1] = 0   */
} rt_closest;
typedef struct rt_closest_info {        /* 40 B */
    int32_t  calls;                     /* calls so far                                                                                 */
    int32_t  _reserved;
    double   lastKernelMs, totalKernelMs;   /* HIP-event time of the launches of the last host-entry call / summed                      */
    uint64_t lastNodeSteps, lastPrimTests;  /* option "closest_count" = 1: node steps and primitive tests (spheres and triangles) of all
                                               points of the last call; else 0                                                          */
} rt_closest_info;
/* Host memory; returns when the results are in out.  The points go through device buffers of the context in slices of "closest_slice"
 * points, sized to min(n, slice).  out: n rt_closest — n * K, point-major, when option "closest_k" is K (K-nearest queries below), the
 * slices then min("closest_slice", 4194304 / K) points.                                                                          */
int rt_closest_points       (rt_ctx* ctx, const rt_ray* points, int n, rt_closest* out);
/* Device memory of the context's GPU (points: n rt_ray, out: n rt_closest — n * K with option "closest_k" = K —, both 16-byte aligned), ordered on the context's stream as
 * rt_trace_rays_device is, with its one synchronisation for the origin bound; rt_closest_info counts the call and keeps the host
 * entry's times.  After a counting call rt_get_closest_info waits for the stream once to fetch the counts.                        */
int rt_closest_points_device(rt_ctx* ctx, const void* points, int n, void* out);
int rt_get_closest_info     (rt_ctx* ctx, rt_closest_info* out);

/* ---- K-nearest queries: every surface within a radius of a point, nearest first, and how many there are -------------------------------
 * Unity's Physics.OverlapSphere beside ClosestPoint: rt_closest_points returns one winner; a capsule pressed into a corner touches two or
 * three faces, the faces that meet at a crease tie bit for bit and only a caller who receives all of them can decide the sign there, and
 * "how many primitives lie within R" is a question of its own (probe culling, level of detail, smoothing a baked field).  No new entry
 * and no new record: the options "closest_k" (K, 1..8 = RT_HITS_MAX, default 1) and "closest_all" (0 or 1, default 0) of rt_set_option /
 * rt_multi_set_option change what rt_closest_points, rt_closest_points_device and rt_multi_closest_points write, and nothing else: every
 * other call ignores them.  At K = 1 and all = 0 the three calls are exactly the closest-point queries above — the same kernel, the
 * same bytes, _reserved 0.  Otherwise they write n * K rt_closest, point-major (record j of point i at out[i * K + j]):
 *
 *   candidates    exactly the closest-point queries': every uploaded sphere and every triangle rt_read_bvh_order lists.  The sphere key
 *   keys          and the seven-region triangle key are those of "closest-point queries", operation for operation.  A candidate counts
 *   records       when k < R * R (the product a float, the comparison strict; a NaN k never counts).  The fields of a record are those
 *                 rt_closest defines: point, dst, normal, side, u, v and the indices of that candidate.
 *   order         ascending (k, kind, primitive): k compares as a float; at equal k a sphere comes before a triangle, then the lower
 *                 uploaded index.  With total = the number of candidates that count, records 0 .. min(total, K) - 1 are the nearest
 *                 candidates in that order; the remaining records are the miss record.
 *   count         _reserved[0] of ALL K records of a point holds the point's count, _reserved[1] = 0.  all = 0: the count is
 *                 min(total, K); a count equal to K means "there may be more".  all = 1: the count is total, the number of ALL
 *                 candidates with k < R * R; the search is then bounded by R alone (with an unbounded R every primitive is examined).
 *                 K = 1 with all = 1 is legal: the closest point plus the overlap count.  Record 0 of any form equals the default
 *                 call's record in every word but _reserved[0].
 *   not searched  R <= 0, R NaN, a point with a NaN or infinite component: K miss records with count 0.
 *   scene, state  the closest-point queries' (scene, state, errors): the queue is settled, the scene made current, the padding widened;
 *   slicing       nothing else moves.  A batch cut anywhere into two calls gives the bits of one; rt_multi is invisible (set the options
 *   errors        with rt_multi_set_option: every context must hold the same K).  The points per launch and per staging slice are
 *                 min("closest_slice", 4194304 / K): the staged results never exceed the 256 MiB of K = 1.
 *   counting      "closest_count" = 1 works in every form and fills rt_closest_info.lastNodeSteps / lastPrimTests.
 *   refusals      "closest_k" outside 1..8 and "closest_all" other than 0 or 1: -2 with a message; the option keeps its value.        */

/* ---- box overlap queries: every surface that touches a box, nearest to its centre first, and how many there are -----------------------
 * Unity's Physics.OverlapBox / CheckBox beside OverlapSphere: which surfaces pass through a trigger volume, a marquee cell, a placement
 * footprint, one voxel of a grid (conservative voxelisation is this query with one box per cell).  A box is not a ball: the sphere around
 * a thin box over-reports.  No new entry and no new record: option "closest_box" (0 or 1, default 0) of rt_set_option /
 * rt_multi_set_option changes how rt_closest_points, rt_closest_points_device and rt_multi_closest_points read their input, and nothing
 * else: every other call ignores it, and at 0 the three calls are exactly what they are without it — the same kernels, the same bytes.
 * At 1 each input rt_ray is an axis-aligned box, and the call answers the K-nearest query of the box's centre RESTRICTED to the candidates
 * that touch the box.  Everything is float32, every product and sum rounded on its own (no FMA); dot, cross, / and sqrtf as above.
 *
 *   input         origin = the centre c, direction = the half-extents h, tMax only a gate; _reserved is not read.  Searched when
 *                 tMax > 0 (not NaN), every component of c and h is finite, and h.x, h.y, h.z >= 0; otherwise K miss records with count
 *                 0, and nothing is read.  lo = c - h, hi = c + h, component-wise, as floats.  h = 0 is legal: a point box.
 *   candidates    every uploaded sphere and every triangle rt_read_bvh_order lists, as for closest points.  intersectMode plays no part
 *                 and no rt_params are needed.
 *   sphere        (centre s, radius R, solid) per axis a: e_a = fmaxf(fmaxf(lo.a - s.a, s.a - hi.a), 0.0f);
 *                 d2 = (e_x * e_x + e_y * e_y) + e_z * e_z; it touches when d2 <= R * R.
 *   triangle      A, eAB, eAC the floats the closest-point query reads, B = A + eAB, C = A + eAC.  It touches when ALL of these hold
 *                 (each is written so that a NaN makes it false):
 *                   1 finite   fabsf of each of the nine coordinates of A, B, C is < 1e30f;
 *                   2 bounds   per axis a: fminf(fminf(A.a, B.a), C.a) <= hi.a && fmaxf(fmaxf(A.a, B.a), C.a) >= lo.a;
 *                   3 plane    v0 = A - c, v1 = B - c, v2 = C - c; n = cross(eAB, eAC); d = dot(n, v0);
 *                              rr = (h.x * fabsf(n.x) + h.y * fabsf(n.y)) + h.z * fabsf(n.z); fabsf(d) <= rr;
 *                   4 edges    for each edge f of f0 = eAB, f1 = eAC - eAB, f2 = eAC and each box axis, with j = 0, 1, 2:
 *                                x: p_j = v_j.z * f.y - v_j.y * f.z, r = h.y * fabsf(f.z) + h.z * fabsf(f.y)
 *                                y: p_j = v_j.x * f.z - v_j.z * f.x, r = h.x * fabsf(f.z) + h.z * fabsf(f.x)
 *                                z: p_j = v_j.y * f.x - v_j.x * f.y, r = h.x * fabsf(f.y) + h.y * fabsf(f.x)
 *                              (all three p_j are computed, none is assumed equal to another)
 *                              fminf(fminf(p0, p1), p2) <= r && fmaxf(fmaxf(p0, p1), p2) >= -r.
 *                 Touching counts: the sets are closed.
 *   key, records  a touching candidate gets the key k and the rt_closest record of the closest-point query OF THE POINT c against it
 *   order, count  (the sphere key and the seven-region triangle key of "closest-point queries", operation for operation).  It counts
 *                 when it touches and k is not NaN; there is no radius.  k can be +inf (a large box far from a surface it still
 *                 reaches: |c - q|^2 overflows): such a candidate counts and is listed like any other, after every finite key.  Order, the K records per box ("closest_k") and _reserved[0] are
 *                 exactly the K-nearest queries': ascending (k, kind, primitive), miss records after min(total, K), the count in all K
 *                 records min(total, K), or total with "closest_all" = 1.  Unlike the defaults, K = 1 with all = 0 writes the count too:
 *                 0 or 1, CheckBox.  K = 1 with all = 1 is a voxel's count plus the nearest surface to the cell's centre.
 *   the tree      plays no part: the same bits whatever the tree, the builder, the leaf size, the node form or the order of the visit.
 *                 The walk skips a child only when its (f32 or f16) box is disjoint from [lo, hi] by exact comparison on some axis, or —
 *                 without "closest_all" — when its squared lower bound from c exceeds max(kth * (1 + 2^-19), 2^-100), the K-nearest
 *                 rule.  The first is safe because of condition 2: a leaf slot's box reaches at least 0.99 * 3e-5 * m beyond its
 *                 triangles' uploaded coordinates (m the largest |coordinate|, the padding the BVH audit enforces), A + (B - A) differs
 *                 from the uploaded B by at most about 2^-22 * m, so the bounds of (A, B, C) as formed above lie inside every box on the
 *                 way down; condition 1 removes the coordinates that padding rule exempts.
 *   limits        float32 decides near-misses: a triangle within about 1e-6 (relative to the coordinates) of touching may go either
 *                 way.  The definition is what the checker restates (tests/overlap_oracle.c).
 *   scene, state  the closest-point queries', unchanged: the origin-bound reduction runs on the centres (inputs with tMax > 0);
 *   slicing       "closest_slice" (min("closest_slice", 4194304 / K) boxes per launch) and rt_multi are invisible, a batch cut anywhere
 *   errors        into two calls gives the bits of one; "closest_count" = 1 fills rt_closest_info.lastNodeSteps / lastPrimTests (every
 *                 sphere and every triangle tested against the box is one primitive test).
 *   refusals      "closest_box" other than 0 or 1: -2 with a message; the option keeps its value.                                     */

/* ---- capsule overlap queries: every surface within reach of a segment, nearest first, and how many there are -------------------------
 * Unity's Physics.OverlapCapsule / CheckCapsule, and the question underneath them: which surface is nearest to a SEGMENT, where on the
 * surface, where on the segment, and how far.  Character controllers, ropes and cables, a limb's bone, depenetration of a capsule,
 * clearance along a straight move.  The ball around a capsule over-reports by the capsule's length; a string of balls along its axis
 * under-reports between them.  No new entry and no new record: option "closest_capsule" (0 or 1, default 0) of rt_set_option /
 * rt_multi_set_option changes how rt_closest_points, rt_closest_points_device and rt_multi_closest_points read their input and what they
 * write, and nothing else: every other call ignores it, and at 0 the three calls are exactly what they are without it — the same kernels,
 * the same bytes.  At 1 each input rt_ray is a segment, and the call answers the K-nearest question for it.  Everything is float32, every
 * product and sum rounded on its own (no FMA); dot, cross, / and sqrtf as in "closest-point queries".
 * clamp01(x) below is x < 0 ? 0 : x > 1 ? 1 : x, two selects: a NaN stays a NaN.
 *
 *   input         origin = endpoint P0, direction = the axis d, P1 = P0 + d as floats, tMax = the reach R (the capsule's radius; +inf for
 *                 unbounded); rt_ray._reserved is not read.  Searched when R > 0 (not NaN) and every component of P0, d and P1 is finite;
 *                 otherwise K miss records with count 0, and nothing is read.  d = 0 is legal: a point.  dd = dot(d, d).
 *   candidates    every uploaded sphere and every triangle rt_read_bvh_order lists, as for closest points.  intersectMode plays no part
 *                 and no rt_params are needed.
 *   triangle      A, eAB, eAC the floats the closest-point query reads.  The key is the minimum of up to six sub-candidates, each a
 *                 (k, s, u, v), formed in this order; a later one replaces the running best only when its k is strictly smaller, and a
 *                 NaN k never replaces anything.  When dd == 0 only the first is formed.
 *                   1 endpoint P0   the closest-point query's seven-region test from P0, operation for operation: (k, u, v); s = 0.
 *                   2 endpoint P1   the same from P1; s = 1.
 *                   3 edge AB       E0 = A, e = eAB;  4 edge AC  E0 = A, e = eAC;  5 edge BC  E0 = A + eAB, e = eAC - eAB.  The clamped
 *                                   closest pair of the segment and the edge E0 + e * t (Ericson, Real-Time Collision Detection 5.1.9):
 *                                     r = P0 - E0;  ee = dot(e, e);  f = dot(e, r);  c = dot(d, r);  b = dot(d, e);
 *                                     den = dd * ee - b * b;
 *                                     s0 = den > 0 ? clamp01((b * f - c * ee) / den) : 0;
 *                                     t0 = (b * s0 + f) / ee;
 *                                     ee == 0 || t0 < 0:  t = 0, s = clamp01(-c / dd)          (a degenerate edge is its point E0)
 *                                     else t0 > 1:        t = 1, s = clamp01((b - c) / dd)
 *                                     else:               t = t0, s = s0                       (a NaN t0 ends here, in a NaN key)
 *                                   (u, v) as the seven-region test reports its edge regions: AB (t, 0), AC (0, t), BC (1 - t, t).
 *                   6 piercing      the two-sided RayTriangle of "multi-hit ray queries" from P0 along d, accepted when |det| >= 1e-6f,
 *                                   t, u, v, w >= 0 and t <= 1: s = t and (u, v) that test's.
 *                 Sub-candidates 3 to 6 form their key from their own (s, u, v): x = P0 + d * s; q = (A + eAB * u) + eAC * v; e = x - q;
 *                 k = dot(e, e).  A piercing segment's k is therefore 0 whenever x and q coincide as floats — on exactly representable
 *                 inputs — and otherwise the tiny square of their rounding, never a constant 0 that no computed pair of points backs:
 *                 the search below prunes by distances between computed points, and a key without them could be pruned by no sound rule.
 *   the record    point = q = (A + eAB * u) + eAC * v; dst = sqrtf(k); normal = rt_hit's shading normal at (u, v); u, v; side = the sign
 *                 of dot(x - q, cross(eAB, eAC)) with x = P0 + d * s, 0 for a zero or NaN result, and 0 when the piercing sub-candidate
 *                 is the one that stands.
 *   sphere        (centre c, radius r, SOLID as in box overlap): t = clamp01(dot(c - P0, d) / dd), t = 0 when dd == 0; x = P0 + d * t;
 *                 m = x - c; len = sqrtf(dot(m, m)); ds = len - r, then ds < 0 ? 0 : ds (fmaxf(len - r, 0) for every number; a NaN stays
 *                 a NaN and never counts); k = ds * ds; s = t.  Record: dst = ds; point = c + m * (r / len); normal as for closest points;
 *                 side = len >= r ? +1 : -1.  For len >= r these are the closest-point query's operations from x.
 *   acceptance    a candidate counts when k < R * R, the product a float and the comparison strict; NaN never counts.
 *   order, count  exactly the K-nearest queries': ascending (k, kind, primitive), miss records after min(total, K), _reserved[0] of all
 *                 K records min(total, K), or total with "closest_all" = 1.  As for boxes, K = 1 with all = 0 writes the count too (0 or
 *                 1: CheckCapsule).  _reserved[1] = the bits of the float s in [0, 1], the parameter of the segment's closest point; 0 in
 *                 a miss record.  (rt_ray: origin, direction and tMax are read as above.  rt_closest._reserved: [0] the count, [1] s.)
 *   a point       with d = 0 every record equals the K-nearest query's of the point P0 with the same R, K and all in every word but
 *                 _reserved, whenever P0 lies on or outside every uploaded sphere (inside one the solid sphere's key is 0).
 *   the tree      plays no part: the same bits whatever the tree, the builder, the leaf size, the node form or the order of the visit.
 *                 The walk skips a child only when the squared distance between its (f32 or f16) box and the segment's own bounds
 *                 [min(P0, P1), max(P0, P1)] — per axis max(lo - segmax, segmin - hi, 0), squared and summed as for closest points —
 *                 exceeds max(kb * (1 + 2^-19), 2^-100), kb = R * R while fewer than K candidates are listed or with "closest_all",
 *                 else the K-th key.  Rounding is monotone, so every x = P0 + d * s with s in [0, 1] lies inside those bounds exactly,
 *                 and every q lies in the triangle's padded box as for closest points: the closest-point proof carries over.
 *   limits        float32 decides: the piercing test refuses segments with |det| < 1e-6f (nearly parallel to the face, or a tiny face
 *                 or axis), and those are answered through the edge and endpoint sub-candidates with a small positive k; a segment
 *                 nearly parallel to an edge cancels in den, and s0 may then be any point of the overlap (the pair is still a pair of
 *                 points of the segment and the edge, so k is never below the true distance by more than rounding, and can exceed it
 *                 by the cancellation).  The definition is what the checker restates (tests/capsule_oracle.c).
 *   scene, state  the closest-point queries', with one change: the origin-bound reduction takes the largest finite |coordinate| of P0
 *   slicing       AND of P0 + d over the inputs with tMax > 0, on the host and on the device path.  "closest_slice"
 *   errors        (min("closest_slice", 4194304 / K) segments per launch) and rt_multi are invisible, a batch cut anywhere into two calls
 *                 gives the bits of one; "closest_count" = 1 fills rt_closest_info.lastNodeSteps / lastPrimTests (one sphere or one
 *                 triangle examined is one primitive test, whatever its sub-candidates).
 *   refusals      "closest_capsule" other than 0 or 1: -2 with a message; 1 while "closest_box" is 1, and "closest_box" = 1 while
 *                 "closest_capsule" is 1: -2 with a message (an input is a box or a segment).  The option keeps its value.            */

/* ---- multi-hit ray queries: the first K surfaces along a ray, in order -----------------------------------------------------------------
 * Beside closest hit (rt_trace_rays) and any hit (rt_occluded): EVERYTHING a ray passes through, nearest first — Unity's
 * Physics.RaycastAll.  Layered picking, layer counts, the thickness of a solid along a ray (entry / exit pairs), point-in-solid by
 * parity, transparency and decal stacks.  The reference's RayTriangle is one-sided (det >= 1E-6) and its RaySphere reports the near root
 * only, so RT_HITS_BOTH defines a two-sided mode from the reference's own expressions.  All of it in float32, every product and sum
 * rounded on its own (no FMA); / and sqrtf are IEEE; the answer is the same bits whatever the tree, the builder, the leaf size, the
 * node form or the order of the visit.
 *
 *   candidates    every uploaded sphere, and every triangle CalculateRayCollision can reach: those a chunk addresses.  The context's
 *                 intersectMode applies as for ray queries (RT_INTERSECT_FLAT_CHUNKS when rt_set_params was never called: a query
 *                 needs no params): in FLAT_CHUNKS mode a triangle counts only if its chunk's RayBoundingBox passes (:279).
 *   triangle      front hit: RayTriangle (:150-174) accepts it — det >= 1e-6f && dst >= 0 && u >= 0 && v >= 0 && w >= 0; side = +1.
 *                 back hit (RT_HITS_BOTH only): the same det, inv = 1.0f / det, dst, u, v, w = 1 - u - v that RayTriangle computes,
 *                 accepted when det <= -1e-6f && dst >= 0 && u >= 0 && v >= 0 && w >= 0; side = -1.  u, v, w keep their meaning (the
 *                 weights of B, C and A of the uploaded triangle), so hitPoint and normal are rt_hit's expressions unchanged.  The
 *                 normal is the normalised interpolation of the vertex normals and is NOT flipped for a back hit: it points to the
 *                 triangle's front side, away from the ray's origin side.
 *   sphere        with RaySphere's (:120-146) oc, a, b, c, disc: entry = (-b - sqrtf(disc)) / (2a), accepted when disc >= 0 and the
 *                 quotient >= 0 (RaySphere itself); side = +1.  Exit (RT_HITS_BOTH only) = (-b + sqrtf(disc)) / (2a) from the same b,
 *                 disc and a, accepted when disc >= 0 and the quotient >= 0; side = -1.  normal = normalize(hitPoint - centre) for
 *                 both (it points outwards).  An origin inside a sphere sees its exit alone.
 *   bound         a hit counts when dst < tMax (strict).  tMax <= 0 or NaN: nothing is traced, K empty records, hitCount = 0.  An
 *                 accepted dst is finite and >= 0; -0.0f is possible.
 *   order         ascending (dst, kind, primitive, side): dst compares as a float (-0.0f == 0.0f); at equal dst a sphere comes before
 *                 a triangle, then the lower uploaded index, then front (+1) before back (-1).  Record 0 therefore equals
 *                 rt_trace_rays' hit, with ONE difference: where several candidates share the closest dst bit for bit, the reference
 *                 keeps the first in its visiting order (spheres in buffer order, then chunk by chunk) and this call keeps the lowest
 *                 (kind, primitive) — the same candidate unless chunks are listed out of the order of their triangles.
 *   output        out holds n * K records, ray-major: records 0 .. min(total, K) - 1 of a ray are its first hits in order, the rest
 *                 are empty: dst = +inf, indices -1, kind = RT_HIT_NONE, side = 0, all else 0 (hitCount apart).
 *   hitCount      the same value in all K records of a ray.  countAll == 0: min(total, K), so hitCount == K means "there may be
 *                 more".  countAll == 1: the number of ALL accepted hits with dst < tMax; the traversal is then bounded by tMax
 *                 alone and cannot stop early.  In RT_HITS_FRONT mode hitCount > 0 exactly when rt_occluded says 1.
 *   defaults      params == NULL: maxHits = RT_HITS_DEFAULT_MAX, RT_HITS_FRONT, countAll 0.
 *   scene, state  as for ray queries: the queue is settled, the scene made current, the box padding widened for the largest finite
 *                 |origin coordinate| among rays with tMax > 0 (the device entry: one small reduction and one synchronisation first).
 *                 Nothing else moves — not the image, feature, filter or other query state, and no rt_stats field except bvhBuilds /
 *                 bvhRebuilds / bvhRepads.  The library's slices ("hits_slice") and rt_multi are invisible; a batch cut anywhere into
 *                 two calls gives the bits of one.
 *   errors        a null handle -1; n == 0 returns 0; maxHits outside 1..RT_HITS_MAX, an unknown mode, countAll neither 0 nor 1, a
 *                 reserved word of params that is not 0, n < 0, a null buffer with n > 0, and for the device entry a pointer of another
 *                 device or one not 16-byte aligned: -2 with a message, and nothing changes.                                         */
enum { RT_HITS_FRONT = 0, RT_HITS_BOTH = 1 };
#define RT_HITS_MAX          8
#define RT_HITS_DEFAULT_MAX  4
typedef struct rt_hits_params {         /* 32 B */
    int32_t maxHits;                    /* K, 1..RT_HITS_MAX: the records per ray                                                       */
    int32_t mode;                       /* RT_HITS_FRONT / RT_HITS_BOTH                                                                 */
    int32_t countAll;                   /* 0 / 1, see hitCount                                                                          */
    int32_t _reserved[5];               /* must be 0                                                                                    */
} rt_hits_params;
typedef struct rt_multihit {            /* 64 B; an empty record: dst = +inf, hitPoint = normal = 0, kind = RT_HIT_NONE, indices -1, u = v = 0, side = 0 */
    float   dst;
    float   hitPoint[3];                /* origin + direction * dst                                                                     */
    float   normal[3];                  /* as rt_hit.normal; not flipped for a back hit                                                 */
    int32_t kind;                       /* RT_HIT_*                                                                                     */
    int32_t primitive;                  /* exactly as in rt_hit                                                                         */
    int32_t chunk;
    int32_t mesh;
    float   u, v;                       /* triangle: RayTriangle's u, v; else 0                                                         */
    int32_t side;                       /* +1 front face / sphere entry, -1 back face / sphere exit, 0 in an empty record               */
    int32_t hitCount;                   /* see above; the same value in all K records of a ray                                          */
    int32_t _reserved;
} rt_multihit;
typedef struct rt_hits_info {           /* 32 B */
    int32_t calls;                      /* calls so far                                                                                 */
    int32_t lastMaxHits, lastMode, lastCountAll;    /* the params of the last call, defaults filled in                                  */
    double  lastKernelMs, totalKernelMs;    /* HIP-event time of the launches of the last host-entry call / summed                      */
} rt_hits_info;
/* Host memory; returns when the results are in out (n * K records).  The rays go through device buffers of the context in slices of
 * "hits_slice" rays, sized to min(n, slice) rays and min(n, slice) * K records.                                                   */
int rt_trace_hits       (rt_ctx* ctx, const rt_ray* rays, int n, const rt_hits_params* params, rt_multihit* out);
/* Device memory of the context's GPU (rays: n rt_ray, out: n * K rt_multihit, both 16-byte aligned), ordered on the context's stream
 * as rt_trace_rays_device is, with its one synchronisation for the origin bound; rt_hits_info counts the call and keeps the host
 * entry's times.                                                                                                                 */
int rt_trace_hits_device(rt_ctx* ctx, const void* rays, int n, const rt_hits_params* params, void* out);
int rt_get_hits_info    (rt_ctx* ctx, rt_hits_info* out);

/* ---- sphere-cast-all: the first K surfaces a swept ball touches, in order ---------------------------------------------------------------
 * The listing form of "sphere casts" above, as the multi-hit ray queries are the listing form of the ray queries: Unity's
 * Physics.SphereCastAll.  Every wall a character's step touches, everything a thick projectile pierces, every blocker of a camera boom,
 * "what else is in the way after the first thing".  K calls of a sphere cast with advancing origins do not answer it: contacts at one t
 * are lost, and it costs K traversals.  No new entry, record or struct: option "hits_sweep" (0 or 1, default 0) of rt_set_option /
 * rt_multi_set_option.  With "hits_sweep" = 1, rt_trace_hits, rt_trace_hits_device and rt_multi_trace_hits read each rt_ray as a sphere
 * cast reads it — the radius r is the float whose bits are rt_ray._reserved — and write n * K rt_multihit records, ray-major.  With the
 * option at 0 the three calls are exactly what they are without it: the same kernels and the same bytes, whatever _reserved holds.
 * Everything is float32, every product and sum rounded on its own (no FMA); / and sqrtf are IEEE.
 *
 *   not traced    tMax <= 0 or NaN, or r <= 0, NaN or infinite: K empty records with hitCount 0, and nothing is read.
 *   candidates    one per primitive at most, and exactly what "sphere casts" defines for that primitive alone.
 *                 A scene sphere: RaySphere with radius R + r, hitPoint and normal as there; feature code 0; no guard.
 *                 A triangle: among its eight feature codes (1, 2 the faces from the front and from behind, 3..5 the edges AB, AC, BC,
 *                 6..8 the vertices A, B, C, each exactly as "sphere casts" writes it, qa = ee * dd - nd * nd and all) take those with
 *                 t < tMax that pass the guard — closest_on_triangle(o + d * t)'s key <= g * g, g = r * (1 + 2^-6).  The triangle's
 *                 candidate is the one with the smallest (t, code); a triangle none of whose features passes is no candidate.
 *                 intersectMode plays no part, and rt_hits_params.mode is validated as ever and then not read: the test is two-sided
 *                 by construction.
 *   order         ascending (t, kind, primitive): t compares as a float (-0.0f == 0.0f); at equal t a sphere comes before a triangle,
 *                 then the lower uploaded index.
 *   records       records 0 .. min(total, K) - 1 of a ray are its first candidates in that order, the rest are rt_multihit's empty
 *                 record.  Words 0..12 (dst .. v) of a filled record are the words the sphere cast's rt_hit has for that candidate:
 *                 dst = t, hitPoint the contact point, normal the CONTACT normal (from the contact to the ball's centre, normalised),
 *                 kind, primitive, chunk, mesh, u, v as there.
 *   side          a scene sphere: +1.  A triangle: the sign of dot(centre - hitPoint, cross(eAB, eAC)) with centre = o + d * t: +1,
 *                 -1, or 0 (also 0 for a NaN) — which side of the face the ball's centre is on at the contact.
 *   hitCount      as in rt_trace_hits: min(total, K), or with countAll = 1 the number of ALL candidates with t < tMax (the traversal
 *                 is then bounded by tMax alone).  The same value in all K records of a ray.
 *   _reserved     the contact's feature code, 0..8.
 *   consequences  Record 0 equals the "sweep" = 1 rt_trace_rays record of the same ray in words 0..12 and in the feature code, and
 *                 hitCount > 0 exactly when the "sweep" = 1 rt_occluded says 1.  The records of a call at K are the first K records of
 *                 a call at any larger K (hitCount apart).  The answer does not depend on the tree, the builder, the leaf size, the
 *                 node form or the visiting order.  The library's slices ("hits_slice") and rt_multi are invisible; a batch cut anywhere
 *                 into two calls gives the bits of one.  Scene and state: as for rt_trace_hits (rt_hits_info counts the call and its
 *                 lastMode reports the params' mode).
 *   limits        all of the sphere casts' limits carry over unchanged: the float32 range of the quadratics, balls that start
 *                 overlapping (a primitive whose contact lies behind the origin reports nothing), origins many radii away.
 *   refusals      "hits_sweep" other than 0 or 1: -2 with a message, and the option keeps its value.  It is independent of "sweep":
 *                 either may be 0 or 1, "sweep" = 1 still changes nothing about rt_trace_hits, and "hits_sweep" = 1 changes nothing
 *                 about any other call.  rt_hits_params is checked as ever (a reserved word that is not 0: -2).                     */

/* ---- feature buffers: albedo, normal, depth and coverage of the first visible surface ---------------------------------
 * What a denoiser, a compositor or an edge-aware filter takes beside the noisy image.  The reference has no such output (its only
 * target is the colour of RayTracing.shader:388); the definition below is this library's, built from the reference's own steps.
 * For pixel (x, y) of feature frame f, with N = numRaysPerPixel:
 *
 *   camera rays   sample s draws its ray exactly as frag does (:377-382), from the PHILOX stream with key (pixelIndex, f), counter
 *                 (block 0, sample s) — whatever rngMode is.  In RT_RNG_PHILOX mode these are, bit for bit, the camera rays the frame
 *                 traces (the same pixel footprint, the same anti-aliasing).  In RT_RNG_PCG mode they are an independent stream of the
 *                 same distribution: the reference chains one PCG state through every bounce of a pixel, so its camera rays cannot be
 *                 reproduced without tracing the paths.  The feature buffers therefore do not depend on rngMode.
 *   surface       the hit at which Trace (:300-352) first reaches its scatter step: the first CalculateRayCollision hit, except that a
 *                 hit on an InvisibleLight material (flag 2) is passed through once as Trace does at bounce 0 (origin = hitPoint +
 *                 dir * 0.001, one more cast, only if maxBounceCount >= 1; the second cast's hit counts whatever its flag).
 *                 intersectMode applies.  No surface = a miss.
 *   per sample    hit: albedo = the material's colour with Trace's checker rule (flag 1: emissionColour where mod2(floor(x)) !=
 *                 mod2(floor(z)), :313-317), normal = the hit's shading normal, depth = sqrt(dot(q, q)) with q = hitPoint - the camera
 *                 ray's origin, coverage = 1.  A miss: 0 in all eight channels.
 *   sum           the fixed tree of the Philox mode (RT_RNG_PHILOX above), each channel on its own; the root is divided by N.
 *                 Plane RT_AOV_ALBEDO = (albedo.rgb, coverage), plane RT_AOV_NORMAL_DEPTH = (normal.xyz, depth), RGBA32F.  The mean
 *                 normal is not normalised and depth is the mean over ALL samples (divide by coverage for the mean over the hits).
 *   accumulate    per plane and channel acc = acc * (1 - w) + cur * w, w = 1 / (k + 1), k = feature frames accumulated so far — the
 *                 running mean of Accumulate.shader:43-54 without its saturate (normals are signed, depths exceed 1).
 *
 * rt_render_aov settles the queue, makes the scene current as a frame does (pending uploads, moved meshes, box padding for the camera),
 * honours rt_set_rows / rt_set_bands and rt_set_stream, and runs one kernel launch per feature frame.  It moves nothing of the image
 * path: resultTexture, currentFrame, numRenderedFrames, rays and the work counters stay (only bvhBuilds / bvhRebuilds / bvhRepads move
 * when the call triggered them, as for ray queries).  The planes are created zeroed at first use and again whenever the strip's size
 * changes (as the accumulation target is); rt_reset_accum leaves them alone, rt_reset_aov zeroes them.  The strip layout of
 * rt_read_aov / rt_copy_aov_to_device is rt_read_accum's (rows*width*4 floats).
 * Errors: null context -1; no params set, n_frames < 0, an unknown plane, a wrong n_floats or a null buffer -2 with a message;
 * n_frames == 0 returns 0.                                                                                                       */
enum { RT_AOV_ALBEDO = 0, RT_AOV_NORMAL_DEPTH = 1, RT_AOV_COUNT = 2 };
typedef struct rt_aov_info {
    int32_t framesAccumulated;          /* feature frames in the planes                                                     */
    int32_t lastSampleLanes;            /* lanes of a wave that shared a pixel's samples in the last launch (16, 4 or 1)      */
    double  lastKernelMs;               /* HIP-event time of the launches of the last rt_render_aov call                     */
    double  totalKernelMs;              /* sum over the calls since the planes were last zeroed                              */
} rt_aov_info;
int rt_render_aov(rt_ctx* ctx, int first_frame, int n_frames);
int rt_read_aov(rt_ctx* ctx, int which, float* rgba, size_t n_floats);
int rt_copy_aov_to_device(rt_ctx* ctx, int which, void* dst_device_ptr, size_t n_floats);
int rt_reset_aov(rt_ctx* ctx);
int rt_get_aov_info(rt_ctx* ctx, rt_aov_info* out);

/* ---- denoiser: an edge-avoiding A-trous wavelet filter guided by the feature buffers --------------------------------------
 * rt_denoise filters the context's current resultTexture into a further RGBA32F plane, the denoised plane, guided by the context's
 * current feature planes: the step between resultTexture and the display blit.  The reference has no such step (its resultTexture goes
 * to the screen as it is, RayTracingManager.cs:84); the definition below is this library's: the edge-avoiding A-trous wavelet transform
 * of Dammertz et al. (HPG 2010) with albedo demodulation, frozen to the bit.  All arithmetic is IEEE float32 without FMA contraction,
 * every '/' a correctly rounded quotient, exp2_ the polynomial of csrc/rt_math.hpp (rtm::exp2_).  Per pixel p, with C = resultTexture
 * (rgb, a), A = plane RT_AOV_ALBEDO (albedo.rgb, coverage), G = plane RT_AOV_NORMAL_DEPTH (n.xyz, z):
 *
 *   demodulate    cov1 = 1.0f - A.w; per channel d = max(A.ch + cov1, 0.01f) and e0.ch = C.ch / d: the sky part of a pixel counts as
 *                 albedo 1.  With demodulate == 0, d = 1 and e0 = C.rgb.
 *   constants     kn = 1.0f / (sigmaNormal * sigmaNormal), kz = 1.0f / (sigmaDepth * sigmaDepth),
 *                 kc_i = (1.0f / (sigmaColour * sigmaColour)) * (float)(1 << (2 * i)): the colour sigma halves every pass, as in the
 *                 paper; per pixel zs = kz / (G_p.w * G_p.w + 1e-6f): the depth difference is relative to the centre's depth.
 *   pass i        for i = 0 .. iterations - 1, with step s = 1 << i: the taps q = p + (dx * s, dy * s), dy = -2..2 outer, dx = -2..2
 *                 inner, in that order; a tap outside the image is skipped, not clamped.  Per tap
 *                     dn2 = (dnx*dnx + dny*dny) + dnz*dnz        (dn = G_p.xyz - G_q.xyz)
 *                     dz  = G_p.w - G_q.w
 *                     dc2 = (dcx*dcx + dcy*dcy) + dcz*dcz        (dc = e_i(p) - e_i(q))
 *                     x   = (dn2*kn + (dz*dz)*zs) + dc2*kc_i
 *                     w   = (h[dy+2] * h[dx+2]) * exp2_(-x)         h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *                 accumulated in tap order: sw = sw + w, s.ch = s.ch + w * e_i(q).ch; then e_{i+1}(p).ch = s.ch / sw.  The centre tap
 *                 has x = 0, so sw >= 9/64.
 *   output        out.ch = e_last.ch * d per channel, out.a = C.a.
 *
 * Non-finite inputs give whatever this arithmetic gives; the call does not fault on them.
 * rt_denoise settles the queue, runs on the context's stream (rt_set_stream) and moves nothing else: resultTexture, currentFrame,
 * numRenderedFrames, the feature planes, rt_aov_info and every rt_stats field stay.  It needs the whole image in one context: a context
 * that rt_set_rows / rt_set_bands has given less returns -2 (use rt_multi_denoise).  The work planes and the denoised plane are created
 * at first use and again when the image size changes.  params == NULL means the defaults: iterations 5 and the values of
 * RT_DENOISE_DEFAULT_* (chosen by the sweep of profiles/denoise_defaults.txt).
 * Errors: null handle -1; no params set, no feature frame accumulated (rt_aov_info.framesAccumulated == 0), iterations outside 1..6,
 * demodulate neither 0 nor 1, a sigma that is <= 0 or not finite, a wrong n_floats / n_pixels, a null buffer, a read before any
 * rt_denoise: -2 with a message, and nothing changed.                                                                             */
typedef struct rt_denoise_params {      /* 32 B */
    int32_t iterations;                 /* 1..6; pass i uses tap spacing 2^i                                                */
    int32_t demodulate;                 /* 0 / 1                                                                            */
    float   sigmaColour, sigmaNormal, sigmaDepth;   /* each finite and > 0                                                  */
    int32_t _reserved[3];
} rt_denoise_params;
#define RT_DENOISE_DEFAULT_ITERATIONS   5
#define RT_DENOISE_DEFAULT_DEMODULATE   0
#define RT_DENOISE_DEFAULT_SIGMA_COLOUR 16.0f
#define RT_DENOISE_DEFAULT_SIGMA_NORMAL 1.0f
#define RT_DENOISE_DEFAULT_SIGMA_DEPTH  0.5f
typedef struct rt_denoise_info {        /* 32 B */
    int32_t iterations;                 /* of the last call                                                                 */
    int32_t demodulate;                 /* of the last call                                                                 */
    int32_t width, height;
    double  lastKernelMs;               /* HIP-event time of the last call's launches                                       */
    double  totalKernelMs;
} rt_denoise_info;
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params);
/* the denoised plane: height*width*4 floats, row 0 = bottom (rt_read_accum's layout for a whole image) */
int rt_read_denoised(rt_ctx* ctx, float* rgba, size_t n_floats);
int rt_copy_denoised_to_device(rt_ctx* ctx, void* dst_device_ptr, size_t n_floats);
/* the display step of rt_read_display applied to the denoised plane (height*width pixels) */
int rt_read_denoised_display(rt_ctx* ctx, uint32_t* rgba8, size_t n_pixels);
int rt_get_denoise_info(rt_ctx* ctx, rt_denoise_info* out);

/* ---- temporal reprojection: carry the image along with a moving camera ---------------------------------------------------
 * rt_temporal is the step between resultTexture and rt_denoise for a camera that moves between displayed frames.  The reference has
 * none: it keeps accumulating, and resultTexture smears.  The caller here resets the accumulation at every pose,
 *     rt_set_params(pose); rt_reset_accum; rt_render(f, k); rt_reset_aov; rt_render_aov(f, k);
 *     rt_temporal(NULL); rt_denoise_temporal(NULL); rt_read_denoised_display(...)
 * and rt_temporal reprojects its previous result into the new view through the first-hit depth, rejects history that belongs to
 * another surface and blends the new samples in with a per-pixel history length (the temporal stage of SVGF, Schied et al., HPG 2017,
 * without its variance estimate).  The step keeps its own state: the temporal colour T (RGBA32F), the history length N (one float per
 * pixel), the guide (normal, depth) and the camera of its previous call.
 * SCOPE: a static scene seen by a moving camera.  There are no motion vectors: the history of a mesh that moved is reprojected as if
 * it had stood still, and the depth and normal test rejects most of it, not all.  rt_reset_temporal is the caller's tool for a scene
 * change.
 *
 * The definition is frozen to the bit.  All arithmetic is IEEE float32 without FMA contraction, every '/' a correctly rounded quotient,
 * sqrt correctly rounded, normalize(v) = v / sqrt(dot(v, v)) (three quotients, csrc/rt_math.hpp), floor the IEEE floor,
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z everywhere, |v|^2 = dot(v, v), and the operations of an expression are evaluated in the
 * order written, left to right within the brackets given.  Inputs of call k: C = resultTexture, A and G = the feature planes, the
 * camera fields of the context's current rt_params M = camLocalToWorld, O = worldSpaceCameraPos, V = viewParams, and from call k - 1
 * the temporal colour T', the history length N', the guide G' and the camera M', O', V'.  Call 0 (the first call, the first after
 * rt_reset_temporal or after a change of the image size) has N' = 0 everywhere, so every pixel takes "no history".  W and H below are
 * (float)width and (float)height.  Per pixel p = (x, y):
 *
 *   surface       cov = A.w, surf = cov > 0; nc = (G.x / cov, G.y / cov, G.z / cov) and zc = G.w / cov if surf, else all 0.
 *   centre ray    frag's ray without jitter (RayTracing.shader:364-372): uv = (((float)x + 0.5f) / W, ((float)y + 0.5f) / H),
 *                 l = ((uv.x - 0.5f) * V.x, (uv.y - 0.5f) * V.y, 1.0f * V.z),
 *                 F.r = ((M[4r] * l.x + M[4r+1] * l.y) + M[4r+2] * l.z) + M[4r+3] * 1.0f for r = 0, 1, 2,  dir = normalize(F - O).
 *   point         X = O + dir * zc (X.i = O.i + dir.i * zc).  Surface: q = X - t' with t' = (M'[3], M'[7], M'[11]), d = X - O',
 *                 ze = sqrt(dot(d, d)).  Sky: q = dir (the sky is at infinity: only the rotation counts).
 *   previous view with c_i = (M'[i], M'[4+i], M'[8+i]), the columns of the upper 3 x 3: l'_i = dot(c_i, q) / dot(c_i, c_i), i = 0, 1, 2.
 *                 s = V'.z / l'_2;  px = ((l'_0 * s) / V'.x + 0.5f) * W - 0.5f,  py = ((l'_1 * s) / V'.y + 0.5f) * H - 0.5f.
 *                 valid = l'_2 > 0 && px > -1 && px < W && py > -1 && py < H (NaN fails each comparison).  Not valid: no tap counts.
 *   taps          x0 = floor(px), fx = px - x0, y0 = floor(py), fy = py - y0.  The taps (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1
 *                 inner, weigh b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy).  A tap counts if it lies inside the image, N'(tap) > 0
 *                 and, for a surface pixel, G'.w > 0 && fabs(G'.w - ze) <= depthTolerance * ze && dot(e, e) <= normalTolerance *
 *                 normalTolerance with e = nc - G'.xyz; for a sky pixel, G'.w == 0.  A tap that does not count is skipped, not
 *                 clamped.  In tap order: sw = sw + b, h.ch = h.ch + b * T'.ch (ch = r, g, b), hn = hn + b * N'.
 *   blend         if sw >= 0.01f: t = hn / sw + 1.0f, n = t < (float)maxHistory ? t : (float)maxHistory, a = 1.0f / n,
 *                 T.ch = (h.ch / sw) * (1.0f - a) + C.ch * a.  Otherwise (no history) n = 1 and T.rgb = C.rgb, the same bits.
 *                 In both cases T.a = C.a and N = n.
 *   afterwards    G' = (nc, zc), the camera becomes the previous camera, T and N become T' and N'.
 *
 * Non-finite inputs give whatever this arithmetic gives; the call does not fault on them and forms no index outside the planes.
 * rt_temporal settles the queue, runs on the context's stream (rt_set_stream) and moves nothing else: resultTexture, currentFrame,
 * numRenderedFrames, the feature planes, rt_aov_info, rt_denoise_info and every rt_stats field stay.  It needs the whole image in one
 * context: a context that rt_set_rows / rt_set_bands has given less returns -2 (use rt_multi_temporal).  Its planes are created at
 * first use and again when the image size changes, which also drops the history.  params == NULL means RT_TEMPORAL_DEFAULT_* (chosen
 * by the sweep of profiles/temporal_defaults.txt).  rt_denoise_temporal is rt_denoise with C = T: the same kernels, the same
 * denoised plane (rt_read_denoised*), the same rt_denoise_info.
 * Errors: null handle -1; no params set, no feature frame accumulated, maxHistory outside 1..4096, a tolerance that is <= 0 or not
 * finite, a wrong n_floats / n_pixels, a null buffer, a read before any rt_temporal (or after rt_reset_temporal),
 * rt_denoise_temporal before any rt_temporal or at another image size: -2 with a message, and nothing changed.                   */
typedef struct rt_temporal_params {     /* 32 B */
    int32_t maxHistory;                 /* 1..4096: the history length is capped here (a = 1 / maxHistory at the least)        */
    float   depthTolerance;             /* relative to the reprojected point's distance; finite and > 0                       */
    float   normalTolerance;            /* on |nc - G'.xyz|; finite and > 0                                                   */
    int32_t _reserved[5];
} rt_temporal_params;
#define RT_TEMPORAL_DEFAULT_MAX_HISTORY      32
#define RT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE  0.05f
#define RT_TEMPORAL_DEFAULT_NORMAL_TOLERANCE 0.5f
typedef struct rt_temporal_info {       /* 32 B */
    int32_t calls;                      /* rt_temporal calls since the history was last dropped                              */
    int32_t width, height;
    int32_t _reserved;
    double  lastKernelMs;               /* HIP-event time of the last call's launch                                          */
    double  totalKernelMs;
} rt_temporal_info;
int rt_temporal(rt_ctx* ctx, const rt_temporal_params* params);
int rt_reset_temporal(rt_ctx* ctx);
/* T: height*width*4 floats, row 0 = bottom (rt_read_accum's layout for a whole image); N: height*width floats */
int rt_read_temporal(rt_ctx* ctx, float* rgba, size_t n_floats);
int rt_read_temporal_history(rt_ctx* ctx, float* n, size_t n_floats);
int rt_copy_temporal_to_device(rt_ctx* ctx, void* dst_device_ptr, size_t n_floats);
/* the display step of rt_read_display applied to T (height*width pixels) */
int rt_read_temporal_display(rt_ctx* ctx, uint32_t* rgba8, size_t n_pixels);
int rt_get_temporal_info(rt_ctx* ctx, rt_temporal_info* out);
int rt_denoise_temporal(rt_ctx* ctx, const rt_denoise_params* params);

/* ---- variance-guided denoiser: an A-trous filter whose colour edge-stop follows the noise ---------------------------------
 * rt_denoise_variance is a second filter beside rt_denoise: the spatial half of SVGF (Schied et al., HPG 2017, 4.2-4.4).  It estimates
 * a per-pixel luminance variance from the image it is given, scales its luminance edge-stop by the square root of that variance and
 * carries the variance through its passes.  It keeps no temporal moments and no state across calls beside its planes.  The definition
 * is frozen to the bit.  All arithmetic follows the denoiser's rules: IEEE float32 without FMA contraction, every '/' and sqrt
 * correctly rounded, exp2_ = rtm::exp2_, operations in the order written.  C is resultTexture (source == 0) or the temporal plane T
 * (source == 1, what rt_denoise_temporal reads); A and G are the feature planes.  Per pixel p:
 *
 *   prep          d and e0.rgb exactly as rt_denoise's demodulate step (d = 1 and e0 = C.rgb with demodulate == 0).
 *   lum           l(e) = (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z
 *   constants     kn, kz and the per-pixel zs exactly as rt_denoise.
 *   estimate      once, on e0: the taps q = p + (dx, dy), dy = -3..3 outer, dx = -3..3 inner; a tap outside the image is skipped.
 *                     g = exp2_(-(dn2*kn + (dz*dz)*zs))       dn2 and dz as in rt_denoise; there is no spatial kernel
 *                 in tap order sg = sg + g, m1 = m1 + g*l_q, m2 = m2 + g*(l_q*l_q) with l_q = l(e0(q)); then mu = m1 / sg,
 *                 v = m2 / sg - mu*mu and var_0(p) = v > 0 ? v : 0 (a select: NaN gives 0).  The centre tap has g = 1.
 *   pass i        for i = 0 .. iterations - 1, with s = 1 << i.
 *                 prefilter: the 3 x 3 taps q = p + (dx, dy) at spacing 1 (whatever s), dy = -1..1 outer, dx inner, that lie inside the
 *                 image, k3 = {1/4, 1/2, 1/4}: pn = pn + (k3[dy+1]*k3[dx+1]) * var_i(q), pd = pd + k3[dy+1]*k3[dx+1]; gv = pn / pd.
 *                 sigma: kl = 1.0f / (sigmaLuminance * sqrt(gv) + 1e-6f).
 *                 taps: rt_denoise's 25 taps at spacing s, in its order, with its skipping rule:
 *                     x = (dn2*kn + (dz*dz)*zs) + fabs(l(e_i(p)) - l(e_i(q))) * kl
 *                     w = (h[dy+2] * h[dx+2]) * exp2_(-x)
 *                 sw = sw + w, s.ch = s.ch + w * e_i(q).ch, sv = sv + (w*w) * var_i(q); then e_{i+1}(p).ch = s.ch / sw and
 *                 var_{i+1}(p) = sv / (sw*sw).  The colour sigma does not halve per pass: the propagated variance shrinks it.
 *   output        out.ch = e_last.ch * d.ch, out.a = C.a, written to the denoised plane: the plane rt_read_denoised,
 *                 rt_copy_denoised_to_device and rt_read_denoised_display read (a read after only this call succeeds).  var_0 is kept in
 *                 the variance plane, height*width floats.
 *
 * Non-finite inputs give whatever this arithmetic gives; the call does not fault on them.
 * rt_denoise_variance settles the queue, runs on the context's stream (rt_set_stream) and moves only the denoised plane, the variance
 * plane, the work planes it shares with rt_denoise (either call rewrites them whole) and rt_vdenoise_info: resultTexture, T and its
 * history, the feature planes, rt_aov_info, rt_denoise_info, rt_temporal_info and every rt_stats field stay.  (The planes are created
 * at first use and again when the image size changes; a re-creation by either filter call restarts rt_denoise_info.totalKernelMs and
 * rt_vdenoise_info.totalKernelMs, the sums over the calls on the planes that exist.)  It needs the whole image in one context (else use
 * rt_multi_denoise_variance).  params == NULL means source 0 and RT_VDENOISE_DEFAULT_* (chosen by the sweep of
 * profiles/vdenoise_defaults.txt).
 * Errors: null handle -1; no params set, no feature frame accumulated, source == 1 before any rt_temporal (or at another image size),
 * a context holding part of the image, iterations outside 1..6, demodulate or source neither 0 nor 1, a sigma that is <= 0 or not
 * finite, a non-zero reserved word, a wrong n_floats, a null buffer, rt_read_variance before any rt_denoise_variance: -2 with a
 * message, and nothing changed.                                                                                                    */
typedef struct rt_vdenoise_params {     /* 32 B */
    int32_t iterations;                 /* 1..6; pass i uses tap spacing 2^i                                                */
    int32_t demodulate;                 /* 0 / 1                                                                            */
    int32_t source;                     /* 0 = resultTexture, 1 = the temporal plane                                        */
    float   sigmaLuminance, sigmaNormal, sigmaDepth;   /* each finite and > 0                                               */
    int32_t _reserved[2];               /* must be 0                                                                        */
} rt_vdenoise_params;
#define RT_VDENOISE_DEFAULT_ITERATIONS      3
#define RT_VDENOISE_DEFAULT_DEMODULATE      1
#define RT_VDENOISE_DEFAULT_SIGMA_LUMINANCE 8.0f
#define RT_VDENOISE_DEFAULT_SIGMA_NORMAL    0.25f
#define RT_VDENOISE_DEFAULT_SIGMA_DEPTH     0.5f
typedef struct rt_vdenoise_info {       /* 32 B */
    int32_t iterations;                 /* of the last call                                                                 */
    int32_t source;                     /* of the last call                                                                 */
    int32_t width, height;
    double  lastKernelMs;               /* HIP-event time of the last call's launches                                       */
    double  totalKernelMs;
} rt_vdenoise_info;
int rt_denoise_variance(rt_ctx* ctx, const rt_vdenoise_params* params);
/* var_0 of the last call: height*width floats, row 0 = bottom (rt_read_accum's row order) */
int rt_read_variance(rt_ctx* ctx, float* var, size_t n_floats);
int rt_copy_variance_to_device(rt_ctx* ctx, void* dst_device_ptr, size_t n_floats);
int rt_get_vdenoise_info(rt_ctx* ctx, rt_vdenoise_info* out);

/* ---- several GPUs of one node behind one handle ---------------------------------------------------------------------
 * The reference renders on one GPU; its path shards into independent pixels (seed = global pixel index + Frame * 719393,
 * RayTracing.shader:360-362; Accumulate.shader is per pixel), so the frame tiles across devices by rows.  An rt_multi owns one
 * rt_ctx per entry of `devices` (a device may appear more than once: several contexts on one GPU, which is how the single-GPU
 * tests exercise this path).  Scene and uniforms are replicated (rt_multi_set_params / rt_multi_upload_* replace the same
 * RayTracingManager calls as their single-device forms); context i renders the 8-row bands b with b % N == i
 * (rt_set_bands(i, N)); rt_multi_render runs the N contexts concurrently for all n_frames and ends with the path's only
 * exchange: one gather of the accumulated strips to the first device (N - 1 peer copies over xGMI, each issued on its source
 * context's stream so that the links run concurrently, joined by events on the first device's stream + a row scatter).  The
 * assembled image is bit-identical to a single-context render (tested).  rt_multi_context gives the per-device context for
 * options, statistics and per-strip read-back.                                                                         */
typedef struct rt_multi rt_multi;
rt_multi*   rt_multi_create(const int* devices, int n_devices);
void        rt_multi_destroy(rt_multi* m);
const char* rt_multi_last_error(const rt_multi* m);
int         rt_multi_count(const rt_multi* m);
rt_ctx*     rt_multi_context(rt_multi* m, int i);
int rt_multi_set_params      (rt_multi* m, const rt_params* params);
int rt_multi_upload_spheres  (rt_multi* m, const rt_sphere*   spheres,  int n);
int rt_multi_upload_triangles(rt_multi* m, const rt_triangle* tris,     int n);
int rt_multi_upload_meshinfo (rt_multi* m, const rt_meshinfo* meshinfo, int n);
/* The on-device geometry pipeline behind the handle (rt_upload_local_meshes / rt_set_mesh_transforms for every context): the local
 * meshes go to every device once, a frame sends the poses (40 B per mesh, RayTracedMesh.cs:36-84: the reference moves meshes every
 * frame) and every device transforms, builds and refits its own copy — no geometry crosses xGMI per frame.                       */
int rt_multi_upload_local_meshes(rt_multi* m, const rt_triangle* local_tris, int n_tris, const rt_local_chunk* chunks, int n_chunks, int n_meshes);
int rt_multi_set_mesh_transforms(rt_multi* m, const rt_mesh_transform* transforms, int n_meshes);
int rt_multi_set_option      (rt_multi* m, const char* name, int value);
int rt_multi_reset_accum     (rt_multi* m);
int rt_multi_render          (rt_multi* m, int first_frame, int n_frames);
/* rt_render_params on every context (its bands, frame f with params[f]), then the one gather.  Same settings rule as rt_render_params
 * (-2 and nothing changed when the entries differ outside the camera fields; new settings act as rt_multi_set_params(&params[0])).  */
int rt_multi_render_params   (rt_multi* m, int first_frame, int n_frames, const rt_params* params);
/* the assembled resultTexture: height*width*4 floats, row 0 = bottom */
int rt_multi_read_accum      (rt_multi* m, float* rgba, size_t n_floats);
/* the assembled image through the display step (rt_read_display's twin: linear -> sRGB8 on the first device; height*width pixels) */
int rt_multi_read_display    (rt_multi* m, uint32_t* rgba8, size_t n_pixels);
/* restore a saved accumulation state (rt_write_accum's twin): the whole image in, every context takes the rows of its bands */
int rt_multi_write_accum     (rt_multi* m, const float* rgba, size_t n_floats, int frames_rendered);
/* rays and work counters summed over the contexts, kernel times = the slowest context's; gather_ms (may be NULL) = wall
 * time of the last gather (copies + scatter)                                                                            */
int rt_multi_get_stats       (rt_multi* m, rt_stats* out, double* gather_ms);
/* How the handle is set up and what a scene change cost: the uploads go to the first context only, which builds the scene once;
 * the other contexts receive the built scene device to device (over xGMI between GPUs) — bvhBuilds counts the builds of ALL
 * contexts since rt_multi_create (one per scene change, whatever N).                                                          */
typedef struct rt_multi_info {
    int32_t numContexts;
    int32_t bvhBuilds;                  /* BVH builds summed over the contexts since rt_multi_create                        */
    double  lastSetupMs;                /* host wall time of the last scene change: build on the first context + fan-out   */
    double  lastGatherMs;               /* host wall time of the last gather: first copy submitted -> image assembled    */
    int32_t device[16];                 /* HIP ordinal of context i (the first 16)                                         */
    int32_t peerAccess[16];             /* 1: the first context's device and context i's read each other's memory directly */
                                        /* (copies go GPU to GPU over xGMI), 0: the runtime stages them; [0] = 1            */
} rt_multi_info;
int rt_multi_get_info        (rt_multi* m, rt_multi_info* out);
/* Ray queries behind the handle (host memory): the batch is cut into one contiguous slice per context, the slices are traced
 * concurrently against each context's copy of the scene and gathered in order — bitwise the single-context result.              */
int rt_multi_trace_rays      (rt_multi* m, const rt_ray* rays, int n, rt_hit* hits);
int rt_multi_occluded        (rt_multi* m, const rt_ray* rays, int n, uint8_t* occluded);
/* Radiance queries behind the handle: the same slices, context i's rays keeping their stream indices (firstIndex + their offset in the
 * batch) — bitwise the single-context result.                                                                                    */
int rt_multi_trace_radiance  (rt_multi* m, const rt_ray* rays, int n, const rt_radiance_params* params, float* rgba);
/* Gather queries behind the handle: the same slices, context i's points keeping their stream indices — bitwise the single-context
 * result.                                                                                                                        */
int rt_multi_gather          (rt_multi* m, const rt_ray* points, int n, const rt_gather_params* params, float* out);
/* Visibility gathers behind the handle: the same slices, context i's points keeping their stream indices — bitwise the single-context
 * result.                                                                                                                        */
int rt_multi_visibility      (rt_multi* m, const rt_ray* points, int n, const rt_visibility_params* params, float* out);
/* Closest-point queries behind the handle: the same slices — bitwise the single-context result.                                   */
int rt_multi_closest_points  (rt_multi* m, const rt_ray* points, int n, rt_closest* out);
/* Multi-hit ray queries behind the handle: the same slices — bitwise the single-context result.                                   */
int rt_multi_trace_hits      (rt_multi* m, const rt_ray* rays, int n, const rt_hits_params* params, rt_multihit* out);
/* Feature buffers behind the handle: every context renders the feature frames of its bands, concurrently; rt_multi_read_aov gathers the
 * strips of one plane to the first device (the gather of rt_multi_render) and returns the assembled plane, height*width*4 floats, row
 * 0 = bottom — bitwise the single-context plane.  rt_multi_reset_aov zeroes the planes of every context.                          */
int rt_multi_render_aov      (rt_multi* m, int first_frame, int n_frames);
int rt_multi_read_aov        (rt_multi* m, int which, float* rgba, size_t n_floats);
int rt_multi_reset_aov       (rt_multi* m);
/* The denoiser behind the handle: the accumulated strips and the strips of both feature planes are gathered to the first device (the
 * gather of rt_multi_render) and the filter of rt_denoise runs there, on the first context's stream — bitwise the single-context result.
 * Every context must hold at least one feature frame.  Per-context state is left alone.                                            */
int rt_multi_denoise              (rt_multi* m, const rt_denoise_params* params);
int rt_multi_read_denoised        (rt_multi* m, float* rgba, size_t n_floats);
int rt_multi_read_denoised_display(rt_multi* m, uint32_t* rgba8, size_t n_pixels);
/* Temporal reprojection behind the handle: the strips of C, A and G are gathered to the first device as for rt_multi_denoise and the
 * step of rt_temporal runs there, on the first context's stream, with the camera of the handle's current params; T, N, the previous
 * guide and the previous camera are kept on the handle — bitwise the single-context result.  rt_multi_denoise_temporal is
 * rt_multi_denoise with C = the handle's T (the feature planes are gathered again); its result is read with rt_multi_read_denoised*. */
int rt_multi_temporal             (rt_multi* m, const rt_temporal_params* params);
int rt_multi_reset_temporal       (rt_multi* m);
int rt_multi_read_temporal        (rt_multi* m, float* rgba, size_t n_floats);
int rt_multi_read_temporal_history(rt_multi* m, float* n, size_t n_floats);
int rt_multi_read_temporal_display(rt_multi* m, uint32_t* rgba8, size_t n_pixels);
int rt_multi_denoise_temporal     (rt_multi* m, const rt_denoise_params* params);
/* The variance-guided denoiser behind the handle: the gather of rt_multi_denoise (source == 0) or of rt_multi_denoise_temporal (source ==
 * 1: C = the handle's T) and rt_denoise_variance's filter on the first device — bitwise the single-context result; the denoised plane is
 * read with rt_multi_read_denoised*, var_0 with rt_multi_read_variance.                                                            */
int rt_multi_denoise_variance     (rt_multi* m, const rt_vdenoise_params* params);
int rt_multi_read_variance        (rt_multi* m, float* var, size_t n_floats);

/* ABI self-description for binding generators / tests. */
int rt_abi_version(void);
int rt_sizeof(const char* struct_name);   /* "rt_material" | "rt_sphere" | "rt_triangle" | "rt_meshinfo" | "rt_params" | "rt_stats" | "rt_mesh_transform" | "rt_local_chunk" | "rt_multi_info" | "rt_ray" | "rt_hit" | "rt_aov_info" | "rt_denoise_params" | "rt_denoise_info" | "rt_temporal_params" | "rt_temporal_info" | "rt_vdenoise_params" | "rt_vdenoise_info" | "rt_radiance_params" | "rt_radiance_info" | "rt_gather_params" | "rt_gather_info" | "rt_visibility_params" | "rt_visibility_info" | "rt_closest" | "rt_closest_info" | "rt_hits_params" | "rt_multihit" | "rt_hits_info" */

#ifdef __cplusplus
}
#endif
#endif /* RT_H_ */
