// rt_ctx.hpp — what the host's translation units share: the context and the multi-device handle behind include/rt.h, the buffers and
// planes they are made of, and the few functions that cross units (namespace rth, hidden: none of it is in the library's symbol table).
//   rt_api.hip      context life cycle, uploads, options, scene builds and refits, the geometry pipeline, plane copies
//   rt_render.hip   frame launches, tile order, camera-ray lists, the submission queue, accumulation target, feature buffers
//   rt_queries.hip  the one path of the six query families
//   rt_filters.hip  the image filters' one host path
//   rt_multi.hip    the rt_multi handle (host code only)
// Host code only: no kernel header is included here; the plain structs a field needs come from rt_types.hpp and bvh.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <ctime>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt.h"
#include "bvh.hpp"
#include "rt_types.hpp"

namespace rtk { struct DeviceScene; }           // rt_kernels.hpp

namespace rth __attribute__((visibility("hidden"))) {

extern thread_local std::string g_create_error;     // (rt_api.hip)
struct ErrOwner { std::string err; };       // what rt_ctx and rt_multi are to fail(): the text rt_last_error / rt_multi_last_error return
int fail(ErrOwner* owner, int code, const char* fmt, ...);

#define RT_HIP(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, -100, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Device memory that is freed with its owner (the owner makes its device current before it goes: rt_destroy, rt_multi_destroy)
template <class T> struct DevBuf {
    T* p = nullptr; size_t cap = 0, used = 0;       // used: elements the last ensure() asked for (what clone_scene copies)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        used = n;
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = std::max<size_t>(n, 1);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; used = 0; }
};

// What the image filters keep between calls (DESIGN.md "The image filters' one host path"): planes made for one image size, and whether
// they hold the result of a call
struct FilterPlanes {
    int w = 0, h = 0;
    bool filled = false;
    size_t pixels() const { return (size_t)w * h; }
};

// THE rule of those planes: `bufs` at W x H are kept while S has that size; else they are re-created, S holds no result and S.new_size()
// resets what S counted over calls
template <class Planes, class... Bufs> hipError_t planes_at(Planes& S, int W, int H, Bufs&... bufs)
{
    if (S.w == W && S.h == H && (... && bufs.p)) return hipSuccess;
    hipError_t e = hipSuccess;
    (void)(... && ((e = bufs.ensure((size_t)W * H)) == hipSuccess));
    if (e != hipSuccess) return e;
    S.w = W; S.h = H; S.filled = false; S.new_size();
    return hipSuccess;
}

// the denoiser's planes (rt_denoise, csrc/rt_denoise.hpp): e_i ping and pong, (d.rgb, C.a), the denoised plane `out` (filled: of a call)
struct DenoisePlanes : FilterPlanes {
    DevBuf<float4> e[2], d, out;
    rt_denoise_info info{};
    hipError_t at(int W, int H) { return planes_at(*this, W, H, e[0], e[1], d, out); }
    void new_size() { info.totalKernelMs = 0; }
};

// what rt_denoise_variance keeps beside the denoiser's planes (csrc/rt_vdenoise.hpp): var_0 of the last call
struct VariancePlane : FilterPlanes {
    DevBuf<float> var;
    rt_vdenoise_info info{};
    hipError_t at(int W, int H) { return planes_at(*this, W, H, var); }
    void new_size() { info.totalKernelMs = 0; }
};

// the state of temporal reprojection (rt_temporal, csrc/rt_temporal.hpp): T, N and the guide G' as ping-pong pairs (`cur` is the pair the
// last call wrote; filled: t[cur], n[cur] and g[cur] hold the result of a call) and that call's camera
struct TemporalPlanes : FilterPlanes {
    DevBuf<float4> t[2], g[2];
    DevBuf<float> n[2];
    int cur = 0;
    rt_params cam{};                // (its camera fields)
    rt_temporal_info info{};
    hipError_t at(int W, int H) { return planes_at(*this, W, H, t[0], t[1], g[0], g[1], n[0], n[1]); }
    void new_size() { info = rt_temporal_info{}; }
    void reset() { filled = false; info.calls = 0; info.lastKernelMs = 0; info.totalKernelMs = 0; }      // rt_reset_temporal: the history is dropped
};

// The rows of the image a context renders (rt_set_rows / rt_set_bands) and so the layout of the planes that hold them: local row ly is
// image row row0 + (ly / 8) * row_stride + ly % 8
struct StripLayout {
    int w = 0, h = 0, row0 = 0, rows = 0, row_stride = 8;
    size_t pixels() const { return (size_t)w * rows; }
    bool operator==(const StripLayout& o) const { return w == o.w && h == o.h && row0 == o.row0 && rows == o.rows && row_stride == o.row_stride; }
};

} // namespace rth

struct rt_ctx : rth::ErrOwner {
    template <class T> using DevBuf = rth::DevBuf<T>;
    using StripLayout = rth::StripLayout;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    rt_params params{};
    bool have_params = false;
    int row0 = 0, nrows = -1;           // -1: whole image
    int band_first = 0, band_stride = 0; // band_stride > 0: interleaved 8-row bands (overrides row0/nrows)

    std::vector<rt_sphere>   h_spheres;
    std::vector<rt_triangle> h_tris;
    std::vector<rt_meshinfo> h_mesh;
    bool scene_dirty = true;
    // option "device_geometry" (rt_upload_triangles from device memory, DESIGN.md "Device-resident triangles")
    int opt_device_geometry = 0;
    bool tris_resident = false;         // the uploaded triangles live in d_raw_tris only (h_tris is empty); n_resident of them
    size_t n_resident = 0;
    bool tree_resident = false;         // the current tree was built from device-resident triangles
    bool deform_pending = false;        // d_raw_tris holds new corners for that tree: prepare_scene updates it in place
    size_t n_tris = 0, n_chunks = 0, n_spheres = 0;     // of the scene on the device (set by build_scene / build_scene_local / clone_scene)
    float sphere_mag = 0.f;                             // largest |coordinate| of a sphere surface point of that scene
    // on-device geometry pipeline (rt_upload_local_meshes / rt_set_mesh_transforms)
    bool geom_local = false, xf_dirty = false;
    uint64_t frames_traced = 0, frames_at_world_build = ~0ull;     // device_bvh = -1: a world-space scene that changes again soon is one that moves
    std::vector<rt_triangle>       h_local_tris;
    std::vector<rt_local_chunk>    h_lchunks;
    std::vector<rt_mesh_transform> h_xf;
    std::vector<float>             mesh_radius;     // largest |local coordinate| * sqrt(3) per mesh
    int n_meshes = 0;
    DevBuf<float> d_local_tris;
    DevBuf<uint32_t> d_tri_mesh, d_tri_chunk, d_tri_rank, d_order;
    DevBuf<rtg::MeshXf> d_xf;
    hipEvent_t evg0 = nullptr, evg1 = nullptr;
    hipEvent_t ev_switch = nullptr;        // rt_set_stream: the work enqueued on the outgoing stream, waited for by the incoming one

    DevBuf<float4> d_sph_geom, d_sph_mat, d_nodes, d_nodes_h, d_tri_geo, d_tri_nrm, d_chunk_mat, d_chunk_box;
    DevBuf<float>  d_raw_tris;
    DevBuf<uint32_t> d_raw_range;
    DevBuf<float4> d_frame, d_accum;
    DevBuf<uint32_t> d_display;
    DevBuf<float4> d_batch;            // per-frame outputs of a multi-frame launch
    DevBuf<uint32_t> d_tile_order, d_tile_cost, d_tile_hist;
    bool lpt_active = true;             // the last launch used (or could have used) a costliest-first order: the automatic kernel choice waits for it
    bool tile_order_valid = false, tile_order_stale = false; int tile_order_n = 0;   // stale: usable, re-measured by the next launch
    StripLayout target;                 // the layout d_frame / d_accum were made for (ensure_targets)
    unsigned int* d_tile_counter = nullptr;
    unsigned long long* d_counters = nullptr;

    rtbvh::Bvh bvh;                 // host builder's result (nodes stay empty after a device build; order / levels / depth are shared)
    size_t n_nodes = 0;             // BVH4 nodes on the device
    rtgb::Workspace bvh_ws;         // device builder's scratch
    float area_at_build = 0.f;      // sum of internal child-box areas right after the last build (refit quality monitor)
    float area_after_refit = 0.f;   // ... after the last refit: written by an asynchronous copy, so it lives in the context, not on a stack
    int opt_device_bvh = -1;        // 1: build the BVH on the device (Morton order + PLOC + collapse), 0: host binned-SAH builder,
                                    // -1: device for the on-device geometry pipeline (meshes that move), host for world-space uploads
                                    // (a static scene is built once and traced for many frames: the SAH tree is traced 4-16 % faster,
                                    // the device build is 25-140x faster)
    int opt_bvh_radius = -16;       // device builder: PLOC search radius; positive: of the first rounds, doubled once a quarter and again once a
                                    // sixteenth of the clusters is left; negative = that radius in every round (default: 16 throughout — with the
                                    // treelet passes on top, profiles/sweep_devtree_r04.txt: wave-level node steps per ray 10.69 / 13.94 on the
                                    // 100k / 1M workloads against 11.16 / 14.52 for 8 widening and 10.64 / 14.91 for the host's SAH tree)
    int opt_peer_copies = 0;        // 1: rt_multi's device-to-device copies take the peer API (hipMemcpyPeerAsync) even between contexts of ONE device
                                    // — the branch a multi-GPU node takes, runnable on a one-GPU box (tests)
    int opt_bvh_treelet_ratio = 8, opt_bvh_treelet_isolate = 1, opt_bvh_treelet_first = 1;      // (tuning of the passes: scale step, large-box isolation, first item size)
    int opt_bvh_treelets = 6;       // device builder: sweep-SAH passes over the clustering's tree, one wave per treelet of <= 64 items (rt_bvh_gpu.hpp step 3c)
    int opt_bvh_top = 0;            // device builder: > 0 = once the bottom-up rounds have left at most this many clusters, the top of the tree is built by
                                    // the host's binned-SAH split search over their boxes (round 3's default 1024: a few hundred KB and about a
                                    // millisecond of host time); 0 (default since round 4) = everything on the device: the treelet passes reach the root
    int opt_rebuild_percent = 200;  // device pipeline: rebuild instead of refit once the internal area exceeds this share of the build's
    int n_cu = 0;
    int opt_kernel = -1;            // -1: auto (k_trace or k_stream, measured per scene), 0: k_trace, 1: k_stream
    int auto_choice = -1; double auto_ms[2] = { -1.0, -1.0 };
    unsigned variants_launched = 0;     // kernel variants that have run at least once in this context (automatic choice: see launch_frames)
    int opt_shade_threshold = 48;
    int opt_tile_sync = 1;
    int opt_fetch_guide = 4;        // k_stream: groups of tiles_per_fetch items while more than this many groups per wave are left (then smaller)
    int opt_fetch_guide_philox = 1; // ... the same in Philox mode
    int opt_tiles_per_fetch = 16;   // k_stream: items a wave reserves per fetch while the queue is long (guided: fewer near the end).  Fixed groups of
                                    // 2 / 4 / 8: 11.89 / 12.17 / 11.65 Grays/s (the tail grows); guided 4 / 8 / 12 / 16 / 24: 12.35 / 12.55 / 12.60 / 12.61 / 12.60.
                                    // 16 = the sub-tiles of one 8x8 tile in a 2x2x16 launch: groups stay tile-aligned (15.31 against 15.26 at 12)
    int opt_compact_nodes = 1;      // k_trace / k_stream: traverse the f16 form of the nodes (Node4h: 5 loads per visit instead of 7)
    int opt_stream_tile = 4;        // k_stream: log2 of the most frames interleaved in a wave (0: 8x8 pixels x 1 frame, 2: 4x4 x 4, 4: 2x2 x 16)
                                    // measured on the 100k-triangle workload: 10.86 / 11.48 / 11.89 Grays/s; with 4 tiles per fetch 12.17
    int opt_node_min = 10;          // k_stream: 4..10 within 0.5 % of each other on the 100k-triangle workload (+7 % over 1); 6 / 8 / 10 on the
                                    // million-triangle one: 11.72 / 11.83 / 11.90 Grays/s
    int opt_blocks_per_cu = 0;      // 0: occupancy API
    int opt_full_sort = 0;          // 1: sort all four children; 0: nearest first only (measured +1 %)
    int opt_tile_lpt = 1;           // k_trace: dispatch the costliest tiles first, using the costs measured by the previous launch
    int opt_frame_batch = 0;        // k_trace: frames per launch in rt_render (0 = auto, 1 = one launch per frame)
    int opt_tile_w_log2 = 3;        // k_trace: tile width 2^n (n = 3: 8x8 tiles)
    int opt_bvh_reinsert = 0;       // BVH builder: insertion-based optimisation passes
    int opt_bvh_bins = 32, opt_bvh_cost_exp = 100;   // BVH builder: SAH bins per axis; exponent (percent) of the count in the SAH cost model
    int opt_max_leaf = 2;           // BVH: triangles per leaf (measured best on the 100k-triangle workload: 2)
    int opt_bvh_collapse = 0;       // host builder: 0 = greedy collapse of the binary tree to 4-wide nodes (open the largest child), 1 / 2 = cost-driven (bvh.cpp;
                                    // measured -4.4 % / -1.5 % on the headline scene, -1.4 % / +1.5 % on the million-triangle one: profiles/bvh_collapse_r04.txt)
    int opt_bvh_node_cost = 130;    // ... with a node step costing this many percent of a triangle test
    int opt_stream_stack = 0;       // k_stream: stack entries per lane kept in LDS; deeper BVHs spill the rest to global memory.  0 = as many as let the
                                    // instantiation's waves per SIMD be resident: 24 entries + the groups' item tables = 25,600 B per workgroup for the six-wave
                                    // PCG / f16-node kernel (six workgroups per CU; 26 entries make it five: -8 %), 30 = 31,744 B for the five-wave ones
    int opt_lds_stack = 0;          // k_trace: stack entries per lane kept in LDS (0 = the BVH's worst case, nothing spills)
    DevBuf<uint32_t> d_gstack;
    // camera rays' candidate lists (rt_primary.hpp): valid for one (params, rows, scene) combination
    DevBuf<uint4> d_primary; DevBuf<float4> d_focus; DevBuf<unsigned int> d_primary_counts;
    std::string primary_key;                        // what the lists were built for (parameters, rows, scene version)
    unsigned long long scene_version = 0;           // bumped whenever the tree or its boxes change (build, refit, re-padding)
    int opt_primary_lists = 1;                      // 1: camera rays of a static camera start from their pixel's candidate leaves (k_stream); 0: always from the root
    DevBuf<float> d_park;              // k_stream, Philox mode: parked sub-stream sums
    std::vector<rtk::CamRecord> h_cams; DevBuf<rtk::CamRecord> d_cams;     // k_cam_stream: the camera table of the last launch (rt_render_params)
    // queries (rt_trace_rays ... rt_trace_hits): staging of the host entries (one slice of rays or points in, one slice of results
    // out, in bytes), the device entries' origin bound, and the timed families' info records (QueryFamily indexes them; closest-point
    // queries and
    // multi-hit queries use calls and the two times of theirs)
    DevBuf<float4> d_q_rays; DevBuf<uint8_t> d_q_out;
    DevBuf<unsigned int> d_q_bound;
    rt_gather_info query_info[5]{};
    // multi-hit ray queries: rays per launch (a slice stages maxHits * 64 B of records per ray), and the params of the last call
    int opt_hits_slice = 1 << 18;
    rt_hits_params hits_last{};
    // closest-point queries: points per launch; 1 = the counting kernel (node steps and primitive tests of a call, summed on the device
    // and fetched by rt_get_closest_info when counts_pending says the last call left some there)
    int opt_closest_slice = 1 << 22, opt_closest_count = 0;
    int opt_sweep = 0;              // 1: the ray queries answer for a ball (csrc/rt_sweep.hpp)
    int opt_hits_sweep = 0;         // 1: the multi-hit ray queries list what a ball touches (csrc/rt_sweep_all.hpp)
    int opt_closest_k = 1, opt_closest_all = 0;     // K-nearest queries: records per point, count every candidate (csrc/rt_nearest.hpp); 1 and 0: k_closest
    int opt_closest_box = 0;                        // box overlap queries: 1 = each input is a box (centre, half-extents), k_overlap (csrc/rt_overlap.hpp)
    int opt_closest_capsule = 0;                    // capsule overlap queries: 1 = each input is a segment (P0, d, reach), k_capsule (csrc/rt_capsule.hpp)
    DevBuf<unsigned long long> d_closest_counts;
    bool closest_counts_pending = false;
    unsigned long long closest_counts[2]{};
    int opt_visibility_slice = 1 << 22; // visibility gathers: points per launch (and per staging slice of the host entry); the result never depends on it
    int opt_gather_slice = 1 << 20;     // gather queries: points per launch (and per staging slice of the host entry); the result never depends on it
    int opt_radiance_slice = 1 << 22;   // radiance queries: rays per launch (and per staging slice of the host entry); the result never depends on it
    // feature buffers (rt_render_aov, csrc/rt_aov.hpp): the two accumulated planes of this context's strip and the layout they were made for
    DevBuf<float4> d_aov[RT_AOV_COUNT];
    StripLayout aov;                    // (meaningful once d_aov[0].p is set: ensure_aov)
    rt_aov_info aov_info{};
    rth::DenoisePlanes dn;              // rt_denoise
    rth::TemporalPlanes tp;             // rt_temporal
    rth::VariancePlane vd;              // rt_denoise_variance
    hipEvent_t ev_dn0 = nullptr, ev_dn1 = nullptr;
    rt_stats stats{};

    // ---- queued submission (rt_submit_frame / rt_wait): frames handed in one by one — the reference's OnRenderImage pattern,
    // RayTracingManager.cs:74-91 — are traced by a worker thread in launches of whatever has queued up while the previous launch ran
    std::thread q_thread; bool q_started = false;
    std::mutex q_mu; std::condition_variable q_cv, q_idle;
    struct QItem { int frame; rt_params p; };   // a queued frame and its uniforms (rt_submit_frame: the params in effect at the tail of the queue)
    std::deque<QItem> q_frames; bool q_busy = false, q_stop = false;
    rt_params q_tail{};                         // the params of the last queued frame (the context's params once the queue has run)
    int q_rc = 0; std::string q_err;
    int opt_queue_depth = 64;       // most frames the worker puts into one launch
    int opt_queue_linger_us = 200;  // after the first frame of an idle queue arrives the worker waits this long for more (a host that submits a burst
                                    // of frames gets one launch for it; a host that submits one frame per display refresh pays 0.2 ms)
};

// ---- several devices behind one handle: frames tile across the GPUs of a node -------------------------------------------
// The path shards into independent pixels (seeds use global pixel coordinates, RayTracing.shader:360-362; accumulation is per
// pixel), so every device holds the whole scene, renders the 8-row bands b with b % N == its rank for all frames, and one
// gather at the end of rt_multi_render brings the strips to the first device: N - 1 peer copies (xGMI point-to-point, each over
// its own link on a fully connected node) and a row scatter.  No other exchange exists on the path.
struct rt_multi : rth::ErrOwner {
    template <class T> using DevBuf = rth::DevBuf<T>;
    std::vector<rt_ctx*> ctx;
    int width = 0, height = 0;
    bool have_params = false;
    DevBuf<float4> d_image, d_staging;          // on the first context's device: the assembled image, the incoming strips
    DevBuf<uint32_t> d_display;                 // ... and its sRGB8 form (rt_multi_read_display)
    DevBuf<float4> d_aov_image;                 // ... the assembled feature plane of the last rt_multi_read_aov
    DevBuf<float4> d_dn_albedo, d_dn_guide;     // ... both assembled feature planes of the last rt_multi_denoise
    rth::DenoisePlanes dn;                      // ... its work planes and the denoised plane
    rth::VariancePlane vd;                      // ... var_0 of the last rt_multi_denoise_variance
    rth::TemporalPlanes tp;                     // ... the state of rt_multi_temporal
    std::vector<hipEvent_t> ev_strip;           // per context: its strip has arrived on the first device (recorded on the SOURCE context's stream)
    int max_rows = 0;
    double lastGatherMs = 0, lastSetupMs = 0;
    bool scene_dirty = true;                    // the first context holds an upload the others have not received yet
    std::vector<int> peer;                      // per context: 1 = the first context's device reads its memory directly (peer access on), 0 = staged by the runtime
};

namespace rth __attribute__((visibility("hidden"))) {

// d = v on the device: ensure, then an asynchronous copy on the context's stream (v must live until the stream is synchronised)
template <class T> hipError_t upload(rt_ctx* c, DevBuf<T>& d, const std::vector<T>& v)
{
    hipError_t e = d.ensure(v.size());
    if (e == hipSuccess && !v.empty()) e = hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream);
    return e;
}

inline double now_ms()
{
    timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
inline float4 f4(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// ---- rt_api.hip: the scene, the rows, the planes ---------------------------------------------------------------------------------------
float camera_magnitude(const rt_params& p);
int prepare_scene(rt_ctx* c);
int cover_origins(rt_ctx* c, float G);
int clone_scene(rt_ctx* dst, rt_ctx* src);
int strip_layout(rt_ctx* c, StripLayout& L);
int create_planes(rt_ctx* c, const StripLayout& L, std::initializer_list<DevBuf<float4>*> planes);
int fill_scene(rt_ctx* c, rtk::DeviceScene& S);
int tile_stack_cap(const rt_ctx* c);
// The traversal stack of a launch of a kernel that traces one query per lane to its end (plan_lane_stack)
struct LaneStack { int cap = 0; size_t lds = 0; uint32_t* gstack = nullptr; unsigned int stride = 0; };
int plan_lane_stack(rt_ctx* c, size_t lanes, LaneStack& st, const char* refuse_4g_for = nullptr);
int sort_tiles_by_cost(rt_ctx* c, uint32_t ntiles);
int copy_plane(ErrOwner* o, const rt_ctx* on, const void* src, size_t expect_floats, const char* shape, void* dst, size_t n_floats, bool to_device);
hipError_t display_plane(rt_ctx* c, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels, float* kernel_ms = nullptr);
int read_srgb8(ErrOwner* o, rt_ctx* on, const float4* plane, size_t pixels, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels);
// Kernels of other families that rt_api.hip instantiates and hands out, as rt_stream_kernels.hip hands out k_stream: the ones that reduce
// over a wave with __shfl_down.  HIP declares it static inline, so the compiler specialises it per unit from all its callers; only
// beside the device builder's library templates (other widths) does it stay general and these kernels keep the code they always had.
const void* trace_kernel(bool counting, bool flat, bool compact, bool spheres_only);       // k_trace
const void* closest_kernel(bool compact, bool counting, bool nearest, bool box, bool capsule);     // k_closest, k_nearest, k_overlap or k_capsule
int cover_origins_device(rt_ctx* c, const float4* rays, int n, bool both_ends);            // k_query_origin_bound

// ---- rt_render.hip: frames, the queue, the feature planes ------------------------------------------------------------------------------
enum class Variant { Fast, Counting, Flat };
int ensure_targets(rt_ctx* c);
bool same_settings(const rt_params& a, const rt_params& b);
int other_settings(const rt_params* params, int n);
void add_launch_stats(rt_stats& sum, const rt_stats& s);
int launch_frames(rt_ctx* c, int first_frame, int n_frames, Variant var, const rt_params* cams = nullptr);
int settle(rt_ctx* c);
#define RT_SETTLE(c) do { const int qr_ = settle(c); if (qr_) return qr_; } while (0)
bool aov_current(const rt_ctx* c, const StripLayout& L);
int ensure_aov(rt_ctx* c);
// rows of rank `rank` of N (bands rank, rank + N, ...: `bands` of them) from its strip to their places in the W x H image, on `stream`
void scatter_bands(hipStream_t stream, const float4* strip, float4* image, int W, int H, int rank, int N, int bands);

// a context's info record (the queue settled first)
template <class Info> int read_info(rt_ctx* c, const Info& info, Info* out)
{
    RT_SETTLE(c);
    if (!out) return fail(c, -2, "null info");
    *out = info;
    return 0;
}

// ---- rt_queries.hip: what a query call is (the path itself: there) -----------------------------------------------------------------------
constexpr int kQuerySlice = 1 << 22;    // rays per launch (and per staging slice of the host entries: 128 MiB of rays, 256 MiB of hits)
enum QueryFamily { kRadiance, kGather, kVisibility, kClosest, kHits, kRays };    // (the first three: the sampled families; the first five are timed and index rt_ctx::query_info)
struct QuerySlice;
struct QueryCall {
    QueryFamily family;
    const char* what;               // the entry's exported name, for messages
    const char* in_word, * out_word;    // what the messages call the items and the results
    int slice;                      // items per launch (and per staging slice of the host entry)
    size_t out_bytes;               // of result per item
    bool out_aligned;               // the device entry wants 16-byte aligned results (all but occlusion bytes)
    const char* refuse_4g_for;      // plan_lane_stack's name for the call; null: ray queries, whose overflow area has no limit
    hipError_t (*launch)(rt_ctx*, const QueryCall&, const QuerySlice&);     // fills the family's Args and launches its kernel
    int sample_lanes_log2;          // S = 16 / 4 / 1 lanes share an item's samples (include/rt.h RT_RNG_PHILOX); ray queries: 0
    rt_gather_params p;             // the sampled families' params, defaults filled in (mode 0 for radiance queries)
    int (*begin)(rt_ctx*);          // what the family does once per call, after the scene is current and before the first launch; may be null
    rt_hits_params h;               // multi-hit queries: their params, defaults filled in
    bool both_ends = false;         // capsule overlap queries: origin + direction is a point of the query too (the origin bound covers it)
    bool sampled() const { return family < kClosest; }      // takes params and draws samples
    bool timed() const { return family != kRays; }          // has an info record with calls and kernel times
};
// A *_call checks the arguments of a call to `what` and describes it (rt_queries.hip "the six descriptions")
using QueryDescribe = int (*)(rt_ctx* c, const char* what, const void* in, int n, const void* params, const void* out, QueryCall& q);
int trace_rays_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* hits, QueryCall& q);
int occluded_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* occluded, QueryCall& q);
int radiance_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* rgba, QueryCall& q);
int gather_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q);
int visibility_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q);
int closest_call(rt_ctx* c, const char* what, const void* points, int n, const void*, const void* out, QueryCall& q);
int hits_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* out, QueryCall& q);
int query_prepare(rt_ctx* c, float G);
int query_entry(rt_ctx* c, QueryDescribe describe, const char* what, bool device, const void* in, int n, const void* params, void* out);

// ---- rt_filters.hip: the image filters' one host path; the handle's two halves of it are rt_multi.hip's -------------------------------
// What a call is called and what its refusals say: `use_instead` is the call a context that holds rows of the image is sent to, `lead`
// what goes before "<rt_temporal> has not been called" when the temporal colour is the source and missing
struct FilterCall { const char* what; const char* use_instead; const char* lead = ""; };

// What a filter runs on: source colour C, albedo A and guide G, all W x H float4 on the current device, the camera `cam` of that image,
// the stream of the launches and the two events that time them
struct FilterInputs {
    const float4* C = nullptr; const float4* A = nullptr; const float4* G = nullptr;
    int W = 0, H = 0;
    const rt_params* cam = nullptr;
    hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    size_t pixels() const { return (size_t)W * H; }
};
int temporal_source(ErrOwner* o, const TemporalPlanes& T, int W, int H, const FilterCall& k, const char* temporal, const char* whose);
int begin_filter(rt_multi* m, const char* what);
int filter_inputs(rt_multi* m, const FilterCall& k, bool from_T, FilterInputs& I);
// (Owner: rt_ctx or rt_multi; both instantiated in rt_filters.hip)
template <class Owner> int denoise_call(Owner* o, const FilterCall& k, bool from_T, const rt_denoise_params* in);
template <class Owner> int temporal_call(Owner* o, const FilterCall& k, const rt_temporal_params* in);
template <class Owner> int denoise_variance_call(Owner* o, const FilterCall& k, const rt_vdenoise_params* in);
int read_filter_plane(ErrOwner* o, const rt_ctx* on, const FilterPlanes& S, const char* call, const void* src, int per, void* dst, size_t n_floats, bool to_device);
int read_filter_display(ErrOwner* o, rt_ctx* on, const FilterPlanes& S, const char* call, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels);

} // namespace rth
