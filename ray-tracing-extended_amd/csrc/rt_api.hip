// rt_api.hip — C-ABI of include/rt.h on top of the HIP kernels (gfx950 only, no CPU fallback).
//
// Host-side counterpart of RayTracingManager.OnRenderImage / InitFrame (RayTracingManager.cs:49-124) below
// the Material.Set* / Graphics.Blit boundary: owns the device copies of the three structured buffers, the
// accumulation target (resultTexture) and the per-frame target (currentFrame).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <vector>

#include "rt_kernels.hpp"
#include "rt_stream.hpp"
namespace rtk {
const void* stream_kernel(bool counting, bool philox, bool compact, bool triangles);        // rt_stream_kernels.hip
const void* cam_stream_kernel(bool philox, bool compact, bool triangles);
}
#include "rt_geom.hpp"
#include "rt_bvh_gpu.hpp"
#include "rt_primary.hpp"
#include "rt_query.hpp"
#include "rt_radiance.hpp"
#include "rt_gather.hpp"
#include "rt_visibility.hpp"
#include "rt_closest.hpp"
#include "rt_multihit.hpp"
#include "rt_sweep.hpp"
#include "rt_nearest.hpp"
#include "rt_overlap.hpp"
#include "rt_aov.hpp"
#include "rt_denoise.hpp"
#include "rt_temporal.hpp"
#include "rt_vdenoise.hpp"

namespace {

thread_local std::string g_create_error;
struct ErrOwner { std::string err; };       // what rt_ctx and rt_multi are to fail(): the text rt_last_error / rt_multi_last_error return

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

} // namespace

struct rt_ctx : ErrOwner {
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
    int opt_closest_k = 1, opt_closest_all = 0;     // K-nearest queries: records per point, count every candidate (csrc/rt_nearest.hpp); 1 and 0: k_closest
    int opt_closest_box = 0;                        // box overlap queries: 1 = each input is a box (centre, half-extents), k_overlap (csrc/rt_overlap.hpp)
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
    DenoisePlanes dn;                   // rt_denoise
    TemporalPlanes tp;                  // rt_temporal
    VariancePlane vd;                   // rt_denoise_variance
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

namespace {

int fail(ErrOwner* owner, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (owner) owner->err = buf; else g_create_error = buf;
    return code;
}

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

void pack_material(const rt_material& m, float4* out)
{
    out[0] = f4(m.colour); out[1] = f4(m.emissionColour); out[2] = f4(m.specularColour);
    out[3] = make_float4(m.emissionStrength, m.smoothness, m.specularProbability, u2f((uint32_t)m.flag));
}

// True when every camera ray starts exactly at worldSpaceCameraPos (frag :377-378 with defocusStrength = +-0): the jitter is
// (finite * +-0) / width = +-0, the basis vectors times it are +-0 when they are finite, and pos + (+-0) = pos bit for bit unless a
// component of pos is -0 (which a +0 turns into +0) or not finite.  The kernels then skip that arithmetic (camera_ray).
bool camera_origin_is_fixed(const rt_params& p)
{
    if (!(p.defocusStrength == 0.0f) || p.width < 1) return false;
    const int basis[6] = { 0, 4, 8, 1, 5, 9 };                   // camera right and up (columns 0 and 1 of camLocalToWorld)
    for (int k : basis) if (!std::isfinite(p.camLocalToWorld[k])) return false;
    for (int a = 0; a < 3; ++a) {
        const float v = p.worldSpaceCameraPos[a];
        if (!std::isfinite(v) || (v == 0.0f && std::signbit(v))) return false;
    }
    return true;
}

// Largest |coordinate| a camera-ray origin can have: camera position plus the defocus disc (frag :377-378).
float camera_magnitude(const rt_params& p)
{
    float m = 0.f;
    for (int a = 0; a < 3; ++a) m = std::max(m, std::fabs(p.worldSpaceCameraPos[a]));
    float jitter = std::fabs(p.defocusStrength) / std::max(1.0f, (float)p.width);
    float axis = 0.f;
    for (int a = 0; a < 3; ++a)
        axis = std::max(axis, std::fabs(p.camLocalToWorld[4 * a]) + std::fabs(p.camLocalToWorld[4 * a + 1]));
    return m + jitter * axis;
}

// Node4 -> Node4h on the device (after a build's upload and after every refit)
int compact_nodes(rt_ctx* c)
{
    const uint32_t nn = (uint32_t)c->n_nodes;
    RT_HIP(c, c->d_nodes_h.ensure((size_t)nn * 8));
    if (nn) {
        hipLaunchKernelGGL(rtg::k_compact_nodes, dim3((nn + 255) / 256), dim3(256), 0, c->stream,
                           reinterpret_cast<const rtbvh::Node4*>(c->d_nodes.p), reinterpret_cast<rtbvh::Node4h*>(c->d_nodes_h.p), nn);
        RT_HIP(c, hipGetLastError());
    }
    return 0;
}

// Bounce rays start on sphere surfaces too (Trace :327): the largest |coordinate| of any sphere surface point.
float sphere_magnitude(const rt_ctx* c)
{
    float m = 0.f;
    for (const rt_sphere& s : c->h_spheres) {
        const float r = std::fabs(s.radius);
        for (int a = 0; a < 3; ++a) { const float v = std::fabs(s.position[a]) + r; if (v > m && v < 3.0e38f) m = v; }
    }
    return m;
}

rtbvh::Tuning bvh_tuning(const rt_ctx* c)
{
    rtbvh::Tuning t;
    t.bins = c->opt_bvh_bins; t.cost_exp_percent = c->opt_bvh_cost_exp; t.reinsert_passes = c->opt_bvh_reinsert; t.max_leaf = c->opt_max_leaf;
    t.collapse_dp = c->opt_bvh_collapse; t.node_cost_percent = c->opt_bvh_node_cost;
    return t;
}

// BVH over the world-space triangles in d_raw_tris, built on the device; then the tracer's triangle records and the f16 nodes.
// Needs d_tri_chunk (0xFFFFFFFF = in no chunk: never hit) and d_tri_rank uploaded.
int device_build(rt_ctx* c, uint32_t nt, float origin_magnitude)
{
    RT_HIP(c, c->d_nodes.ensure(((size_t)nt + 1) * 8)); RT_HIP(c, c->d_order.ensure(nt));
    RT_HIP(c, c->d_tri_geo.ensure(3 * (size_t)nt)); RT_HIP(c, c->d_tri_nrm.ensure(3 * (size_t)nt));
    RT_HIP(c, hipEventRecord(c->evg0, c->stream));
    rtgb::Result res;
    RT_HIP(c, rtgb::build(c->stream, c->d_raw_tris.p, nt, origin_magnitude, c->opt_bvh_radius, c->bvh_ws, reinterpret_cast<rtbvh::Node4*>(c->d_nodes.p), c->d_order.p, res,
                          (uint32_t)c->opt_bvh_top, bvh_tuning(c), c->opt_bvh_treelets, c->opt_bvh_treelet_ratio, c->opt_bvh_treelet_isolate, c->opt_bvh_treelet_first));
    c->bvh.nodes.clear(); c->bvh.order.clear();
    c->n_nodes = res.n_nodes; c->bvh.levelStart = res.level_start; c->bvh.maxStack = res.max_stack; c->bvh.magnitude = res.magnitude;
    c->bvh.depth = res.levels;
    if (nt) {
        hipLaunchKernelGGL(rtg::k_relayout, dim3((nt + 255) / 256), dim3(256), 0, c->stream,
                           c->d_raw_tris.p, c->d_order.p, c->d_tri_chunk.p, c->d_tri_rank.p, c->d_tri_geo.p, c->d_tri_nrm.p, nt);
        RT_HIP(c, hipGetLastError());
    }
    { int r = compact_nodes(c); if (r) return r; }
    RT_HIP(c, hipEventRecord(c->evg1, c->stream));
    RT_HIP(c, rtgb::internal_area(c->stream, reinterpret_cast<const rtbvh::Node4*>(c->d_nodes.p), (uint32_t)c->n_nodes, c->bvh_ws, c->area_at_build));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->evg0, c->evg1));
    c->stats.lastBvhBuildMs = ms; c->stats.bvhBuiltOnDevice = 1; c->stats.bvhBuilds++;
    return 0;
}

// BVH over n triangles (triangle i's corners at positions + i * stride floats), built by the host's binned-SAH builder; then on the
// device the nodes, d_order (BVH order -> uploaded triangle: through live_map for world-space uploads, the identity for local ones),
// the f16 nodes, the tracer's triangle records and the internal area.  Needs d_raw_tris, d_tri_chunk and d_tri_rank uploaded.
int host_build(rt_ctx* c, const float* positions, int stride, uint32_t n, const uint32_t* live_map, float G)
{
    const double t0 = now_ms();
    rtbvh::build(positions, stride, n, G, bvh_tuning(c), c->bvh);
    c->stats.lastBvhBuildMs = now_ms() - t0; c->stats.bvhBuilds++;
    c->n_nodes = c->bvh.nodes.size();
    RT_HIP(c, c->d_nodes.ensure(c->bvh.nodes.size() * 8));
    if (!c->bvh.nodes.empty())
        RT_HIP(c, hipMemcpyAsync(c->d_nodes.p, c->bvh.nodes.data(), c->bvh.nodes.size() * sizeof(rtbvh::Node4), hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> order_raw(live_map ? n : 0);      // (n > 0 means a tree: internal_area below synchronises before it dies)
    for (size_t i = 0; i < order_raw.size(); ++i) order_raw[i] = live_map[c->bvh.order[i]];
    RT_HIP(c, upload(c, c->d_order, live_map ? order_raw : c->bvh.order));
    { int r = compact_nodes(c); if (r) return r; }
    // the records: edge vectors and their cross product are the operands of RayTriangle (RayTracing.shader:152-154), evaluated once
    RT_HIP(c, c->d_tri_geo.ensure(3 * (size_t)n)); RT_HIP(c, c->d_tri_nrm.ensure(3 * (size_t)n));
    if (n) {
        hipLaunchKernelGGL(rtg::k_relayout, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                           c->d_raw_tris.p, c->d_order.p, c->d_tri_chunk.p, c->d_tri_rank.p, c->d_tri_geo.p, c->d_tri_nrm.p, n);
        RT_HIP(c, hipGetLastError());
    }
    RT_HIP(c, rtgb::internal_area(c->stream, reinterpret_cast<const rtbvh::Node4*>(c->d_nodes.p), (uint32_t)c->n_nodes, c->bvh_ws, c->area_at_build));
    return 0;
}

int upload_spheres_and_materials(rt_ctx* c)
{
    const size_t ns = c->h_spheres.size();
    std::vector<float4> sg(ns), sm(4 * ns);
    for (size_t i = 0; i < ns; ++i) {
        const rt_sphere& s = c->h_spheres[i];
        sg[i] = make_float4(s.position[0], s.position[1], s.position[2], s.radius);
        pack_material(s.material, &sm[4 * i]);
    }
    RT_HIP(c, upload(c, c->d_sph_geom, sg)); RT_HIP(c, upload(c, c->d_sph_mat, sm));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->stats.numSpheres = (int)ns;
    return 0;
}

// Triangles of the world-space upload: in h_tris, or in d_raw_tris alone after an upload from device memory
size_t world_tri_count(const rt_ctx* c) { return c->tris_resident ? c->n_resident : c->h_tris.size(); }

// The end of a build: the scene's figures and the counts the launches read.  A new scene starts without a tile order; a rebuild of
// meshes that moved keeps the last one as a predictor, re-measured by the next launch.
void finish_build(rt_ctx* c, bool rebuild = false)
{
    const size_t nt = c->geom_local ? c->h_local_tris.size() : world_tri_count(c), nm = c->geom_local ? c->h_lchunks.size() : c->h_mesh.size();
    c->stats.numSpheres = (int)c->h_spheres.size(); c->stats.numTriangles = (int)nt; c->stats.numMeshChunks = (int)nm;
    c->stats.numBvhNodes = (int)c->n_nodes; c->stats.bvhMaxStack = c->bvh.maxStack; c->stats.bvhInternalArea = c->area_at_build;
    c->n_spheres = c->h_spheres.size(); c->n_tris = nt; c->n_chunks = nm; c->sphere_mag = sphere_magnitude(c);
    c->scene_dirty = false; c->xf_dirty = false; c->scene_version++;
    if (rebuild) c->tile_order_stale = true;
    else c->tile_order_valid = false;
}

// Re-layout of the uploaded buffers + BVH build.
int build_scene(rt_ctx* c)
{
    const size_t nt = world_tri_count(c), nm = c->h_mesh.size();
    if (nt > (1u << 28)) return fail(c, -3, "too many triangles (%zu)", nt);
    // triangle -> chunk map; every triangle the shader can reach belongs to exactly the chunk ranges given.  Equal-distance hits: the
    // reference keeps the triangle its loops reach first — chunks in AllMeshInfo order, triangles in order inside the chunk
    // (CalculateRayCollision :276-293).  That visiting rank, not the buffer index, is the tie-break key.
    std::vector<uint32_t> chunk_of(nt, 0xFFFFFFFFu), visit_rank(nt, 0xFFFFFFFFu);
    uint32_t rank = 0;
    for (size_t m = 0; m < nm; ++m) {
        const rt_meshinfo& mi = c->h_mesh[m];
        if ((uint64_t)mi.firstTriangleIndex + mi.numTriangles > nt)
            return fail(c, -4, "meshinfo[%zu] addresses triangles [%u,%u) beyond the %zu uploaded", m,
                        mi.firstTriangleIndex, mi.firstTriangleIndex + mi.numTriangles, nt);
        for (uint32_t i = 0; i < mi.numTriangles; ++i) {
            uint32_t& slot = chunk_of[mi.firstTriangleIndex + i];
            if (slot != 0xFFFFFFFFu)
                return fail(c, -5, "triangle %u is referenced by chunks %u and %zu (overlapping chunk ranges are not supported)",
                            mi.firstTriangleIndex + i, slot, m);
            slot = (uint32_t)m; visit_rank[mi.firstTriangleIndex + i] = rank++;
        }
    }
    // triangles outside every chunk are never visited by the shader: leave them out of the hierarchy
    std::vector<uint32_t> live; live.reserve(nt);
    for (size_t t = 0; t < nt; ++t) if (chunk_of[t] != 0xFFFFFFFFu) live.push_back((uint32_t)t);
    { int r = upload_spheres_and_materials(c); if (r) return r; }
    std::vector<float4> cm(4 * nm), cb(2 * nm);
    std::vector<uint32_t> range(2 * nm);
    for (size_t m = 0; m < nm; ++m) {
        const rt_meshinfo& mi = c->h_mesh[m];
        pack_material(mi.material, &cm[4 * m]);
        cb[2 * m]     = make_float4(mi.boundsMin[0], mi.boundsMin[1], mi.boundsMin[2], 0.f);
        cb[2 * m + 1] = make_float4(mi.boundsMax[0], mi.boundsMax[1], mi.boundsMax[2], 0.f);
        range[2 * m] = mi.firstTriangleIndex; range[2 * m + 1] = mi.numTriangles;
    }
    RT_HIP(c, upload(c, c->d_chunk_mat, cm)); RT_HIP(c, upload(c, c->d_chunk_box, cb)); RT_HIP(c, upload(c, c->d_raw_range, range));
    // (resident triangles are in d_raw_tris already: rt_upload_triangles copied them there, device to device)
    if (!c->tris_resident) {
        RT_HIP(c, c->d_raw_tris.ensure(nt * 18));
        if (nt) RT_HIP(c, hipMemcpyAsync(c->d_raw_tris.p, c->h_tris.data(), nt * sizeof(rt_triangle), hipMemcpyHostToDevice, c->stream));
    }
    RT_HIP(c, upload(c, c->d_tri_chunk, chunk_of)); RT_HIP(c, upload(c, c->d_tri_rank, visit_rank));     // (what k_relayout reads)
    // headroom: the boxes are padded for ray origins up to twice as far out as the camera and the spheres are now (the term is
    // 2e-6 * G), so a camera that drifts away from the geometry widens the padding (repad_boxes) once per doubling, not per frame
    const float origin_mag = 2.0f * std::max(camera_magnitude(c->params), sphere_magnitude(c));
    c->stats.bvhBuiltOnDevice = 0;
    // device_bvh = -1: the first build of a world-space scene is the host's (a static scene is built once); a scene that is uploaded
    // again within 16 traced frames of its last build is being animated the reference's way — the whole scene re-sent every frame,
    // RayTracedMesh.cs:36-84 — and a 50-600 ms host build per frame would dwarf the trace: those builds go to the device (2.5-5.4 ms)
    const bool moving = c->opt_device_bvh == -1 && c->frames_at_world_build != ~0ull && c->frames_traced - c->frames_at_world_build <= 16;
    c->frames_at_world_build = c->frames_traced;
    int r;
    c->deform_pending = false; c->tree_resident = c->tris_resident && nt > 0;
    // resident triangles: the host builder has no positions to read, so the tree is the device builder's whatever device_bvh says
    if ((c->opt_device_bvh == 1 || moving || c->tris_resident) && nt > 0) {
        // the device builder takes every uploaded triangle; one that belongs to no chunk gets NaN records (k_relayout) and can never be hit
        r = device_build(c, (uint32_t)nt, origin_mag);
    } else {
        std::vector<float> pos(9 * live.size());
        for (size_t i = 0; i < live.size(); ++i) std::memcpy(&pos[9 * i], c->h_tris[live[i]].posA, 36);
        r = host_build(c, pos.data(), 9, (uint32_t)live.size(), live.data(), origin_mag);
        if (live.empty()) c->bvh.magnitude = origin_mag;        // no tree: only the trigger of repad_boxes looks at it
    }
    if (r) return r;
    RT_HIP(c, hipStreamSynchronize(c->stream));     // host staging vectors die here
    finish_build(c);
    return 0;
}

// Bottom-up refit of the tree's boxes from the world-space triangles in d_raw_tris (k_refit_level writes the padded leaf boxes a build
// for magnitude G would), then the f16 form of the nodes.
int refit_tree(rt_ctx* c, float G)
{
    for (int L = (int)c->bvh.levelStart.size() - 2; L >= 0; --L) {
        const uint32_t n0 = c->bvh.levelStart[L], n1 = c->bvh.levelStart[L + 1];
        if (n1 > n0)
            hipLaunchKernelGGL(rtg::k_refit_level, dim3(((n1 - n0) * 4 + 255) / 256), dim3(256), 0, c->stream,
                               reinterpret_cast<rtbvh::Node4*>(c->d_nodes.p), n0, n1, c->d_raw_tris.p, c->d_order.p, G);
    }
    RT_HIP(c, hipGetLastError());
    return compact_nodes(c);
}

// World-space uploads: a ray origin (camera, defocus disc, sphere surface) has moved beyond the magnitude G the boxes were padded
// for (pad = 3e-5 |coord| + 2e-6 G, bvh.cpp pad_box).  The tree stays: its boxes are refitted with the new G — a few small launches
// instead of a host rebuild and a re-upload of every record.
int repad_boxes(rt_ctx* c, float G)
{
    if (c->n_nodes && c->bvh.levelStart.size() >= 2) { int r = refit_tree(c, G); if (r) return r; }
    c->bvh.magnitude = G;
    c->stats.bvhRepads++; c->scene_version++;
    return 0;
}

// Device-resident triangles that deformed (rt_upload_triangles put new corners for the current tree into d_raw_tris): the tracer's
// records are rewritten in BVH order (k_deform_update), the boxes refitted level by level for the padding the tree has, and the
// refitted tree's internal area decides, by the local meshes' rule, whether the device builder replaces it.
int deform_update(rt_ctx* c)
{
    const uint32_t nt = (uint32_t)c->n_tris;
    c->deform_pending = false;
    RT_HIP(c, c->d_q_bound.ensure(1));
    RT_HIP(c, hipEventRecord(c->evg0, c->stream));
    RT_HIP(c, hipMemsetAsync(c->d_q_bound.p, 0, sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(rtg::k_deform_update, dim3((nt + 255) / 256), dim3(256), 0, c->stream,
                       c->d_raw_tris.p, c->d_order.p, c->d_tri_geo.p, c->d_tri_nrm.p, nt, c->d_q_bound.p);
    RT_HIP(c, hipGetLastError());
    // bounce rays start on the triangles: the padding's magnitude covers the new corners as a build's would (4 bytes back, one wait)
    unsigned int mag_bits = 0;
    RT_HIP(c, hipMemcpyAsync(&mag_bits, c->d_q_bound.p, sizeof mag_bits, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->bvh.magnitude = std::max(c->bvh.magnitude, u2f(mag_bits));
    { int r = refit_tree(c, c->bvh.magnitude); if (r) return r; }
    const bool check_area = c->opt_rebuild_percent > 0 && c->area_at_build > 0.f;
    if (check_area) RT_HIP(c, rtgb::internal_area_async(c->stream, reinterpret_cast<const rtbvh::Node4*>(c->d_nodes.p), (uint32_t)c->n_nodes, c->bvh_ws, &c->area_after_refit));
    RT_HIP(c, hipEventRecord(c->evg1, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->evg0, c->evg1));
    c->stats.lastGeometryMs = ms; c->scene_version++;
    if (check_area) {
        const float area = c->area_after_refit;
        c->stats.refitAreaRatio = area / c->area_at_build;
        if (c->stats.refitAreaRatio > (float)c->opt_rebuild_percent / 100.0f) {    // (the ratio, not area_at_build * percent: that product overflows for a tree of 1e36)
            int r = device_build(c, nt, std::max(c->bvh.magnitude, 2.0f * std::max(camera_magnitude(c->params), c->sphere_mag))); if (r) return r;
            RT_HIP(c, hipStreamSynchronize(c->stream));
            c->stats.bvhRebuilds++;
            finish_build(c, true);
        }
    }
    return 0;
}

// ---- on-device geometry pipeline -------------------------------------------------------------------------------
// Conservative bound of |coordinate| over camera-ray origins and the transformed meshes (box padding, bvh.cpp pad_box).
float local_scene_magnitude(const rt_ctx* c)
{
    float G = std::max(camera_magnitude(c->params), sphere_magnitude(c));
    for (int m = 0; m < c->n_meshes; ++m) {
        const rt_mesh_transform& t = c->h_xf[m];
        float p = std::max(std::fabs(t.position[0]), std::max(std::fabs(t.position[1]), std::fabs(t.position[2])));
        float sc = std::max(std::fabs(t.lossyScale[0]), std::max(std::fabs(t.lossyScale[1]), std::fabs(t.lossyScale[2])));
        // a quaternion q = s u (u of unit length) turns p into (1 - s^2) p + s^2 R_u p, at most |1 - s^2| + s^2 times as long: the ABI
        // takes any quaternion.  Within half a percent of unit length the 1.01 covers it and G is what it always was.
        const float q2 = t.rotation[0] * t.rotation[0] + t.rotation[1] * t.rotation[1] + t.rotation[2] * t.rotation[2] + t.rotation[3] * t.rotation[3];
        const float stretch = std::fabs(1.0f - q2) + q2;
        G = std::max(G, p + 1.01f * (stretch > 1.005f ? stretch : 1.0f) * sc * c->mesh_radius[m]);
    }
    return G;
}

// transform + chunk bounds (+ re-layout and refit when the BVH topology already exists).  min_G: ray origins beyond the scene's own
// (a ray query's) that the padding must cover as well
int run_geometry_kernels(rt_ctx* c, bool have_bvh, float min_G = 0.f)
{
    const uint32_t nt = (uint32_t)c->h_local_tris.size(), nm = (uint32_t)c->h_lchunks.size();
    std::vector<rtg::MeshXf> xf(c->n_meshes);
    for (int m = 0; m < c->n_meshes; ++m) {
        const rt_mesh_transform& t = c->h_xf[m];
        xf[m] = { t.position[0], t.position[1], t.position[2], t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3],
                  t.lossyScale[0], t.lossyScale[1], t.lossyScale[2] };
    }
    RT_HIP(c, upload(c, c->d_xf, xf));
    RT_HIP(c, hipEventRecord(c->evg0, c->stream));
    if (nt) {
        hipLaunchKernelGGL(rtg::k_transform, dim3((nt + 255) / 256), dim3(256), 0, c->stream,
                           c->d_local_tris.p, c->d_tri_mesh.p, c->d_xf.p, c->d_raw_tris.p, nt);
        hipLaunchKernelGGL(rtg::k_chunk_bounds, dim3((nm + 255) / 256), dim3(256), 0, c->stream,
                           c->d_raw_tris.p, c->d_raw_range.p, c->d_chunk_box.p, nm);
    }
    if (have_bvh && nt) {
        hipLaunchKernelGGL(rtg::k_relayout, dim3((nt + 255) / 256), dim3(256), 0, c->stream,
                           c->d_raw_tris.p, c->d_order.p, c->d_tri_chunk.p, c->d_tri_rank.p, c->d_tri_geo.p, c->d_tri_nrm.p, nt);
        const float G = std::max(std::max(c->bvh.magnitude, local_scene_magnitude(c)), min_G);
        c->bvh.magnitude = G;
        { int r = refit_tree(c, G); if (r) return r; }
    }
    RT_HIP(c, hipGetLastError());
    // a refit keeps the topology: meshes that moved apart leave boxes that overlap more and more.  The refitted tree's internal area is
    // summed in the same pass (one more small kernel and a 4-byte copy before the one synchronisation, inside lastGeometryMs); once it
    // has grown past the threshold the tree is rebuilt on the device (cheaper than one frame) instead of refitted.
    const bool check_area = have_bvh && nt && c->opt_device_bvh != 0 && c->opt_rebuild_percent > 0 && c->area_at_build > 0.f;
    if (check_area) RT_HIP(c, rtgb::internal_area_async(c->stream, reinterpret_cast<const rtbvh::Node4*>(c->d_nodes.p), (uint32_t)c->n_nodes, c->bvh_ws, &c->area_after_refit));
    RT_HIP(c, hipEventRecord(c->evg1, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->evg0, c->evg1));
    c->stats.lastGeometryMs = ms; c->scene_version++;
    if (check_area) {
        const float area = c->area_after_refit;
        c->stats.refitAreaRatio = area / c->area_at_build;
        if (c->stats.refitAreaRatio > (float)c->opt_rebuild_percent / 100.0f) {    // (the ratio, not area_at_build * percent: that product overflows for a tree of 1e36)
            int r = device_build(c, nt, std::max(local_scene_magnitude(c), min_G)); if (r) return r;
            c->stats.bvhRebuilds++;
            finish_build(c, true);
        }
    }
    return 0;
}

int build_scene_local(rt_ctx* c)
{
    const size_t nt = c->h_local_tris.size(), nm = c->h_lchunks.size();
    if ((int)c->h_xf.size() != c->n_meshes) return fail(c, -2, "rt_set_mesh_transforms has not been called for the %d meshes", c->n_meshes);
    { int r = upload_spheres_and_materials(c); if (r) return r; }
    std::vector<uint32_t> tri_mesh(nt), tri_chunk(nt), tri_rank(nt), range(2 * nm);
    std::vector<float4> cm(4 * nm);
    uint32_t rank = 0;
    for (size_t m = 0; m < nm; ++m) {
        const rt_local_chunk& ch = c->h_lchunks[m];
        for (uint32_t i = 0; i < ch.numTriangles; ++i) {
            tri_mesh[ch.firstTriangleIndex + i] = ch.meshIndex; tri_chunk[ch.firstTriangleIndex + i] = (uint32_t)m;
            tri_rank[ch.firstTriangleIndex + i] = rank++;         // the reference's visiting order (chunk list order, then in-chunk order)
        }
        range[2 * m] = ch.firstTriangleIndex; range[2 * m + 1] = ch.numTriangles;
        pack_material(ch.material, &cm[4 * m]);
    }
    RT_HIP(c, upload(c, c->d_tri_mesh, tri_mesh)); RT_HIP(c, upload(c, c->d_tri_chunk, tri_chunk)); RT_HIP(c, upload(c, c->d_tri_rank, tri_rank));
    RT_HIP(c, upload(c, c->d_raw_range, range)); RT_HIP(c, upload(c, c->d_chunk_mat, cm));
    RT_HIP(c, c->d_local_tris.ensure(nt * 18)); RT_HIP(c, c->d_raw_tris.ensure(nt * 18)); RT_HIP(c, c->d_chunk_box.ensure(2 * nm));
    if (nt) RT_HIP(c, hipMemcpyAsync(c->d_local_tris.p, c->h_local_tris.data(), nt * sizeof(rt_triangle), hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    int r = run_geometry_kernels(c, false);
    if (r) return r;
    c->stats.bvhBuiltOnDevice = 0;
    if (c->opt_device_bvh != 0 && nt > 0) {
        // topology on the device from the world triangles the transform kernel just wrote: nothing goes back to the host
        r = device_build(c, (uint32_t)nt, local_scene_magnitude(c));
    } else {
        // world positions (device) -> host, for the one-off topology build
        std::vector<rt_triangle> world(nt);
        if (nt) RT_HIP(c, hipMemcpy(world.data(), c->d_raw_tris.p, nt * sizeof(rt_triangle), hipMemcpyDeviceToHost));
        r = host_build(c, nt ? world[0].posA : nullptr, 18, (uint32_t)nt, nullptr, local_scene_magnitude(c));
    }
    if (r) return r;
    RT_HIP(c, hipStreamSynchronize(c->stream));
    finish_build(c);
    return 0;
}

// Make the device's scene current for c->params: build what was uploaded, move the meshes, or widen the box padding when a ray origin
// has moved beyond it
int prepare_scene(rt_ctx* c)
{
    if (c->geom_local) {
        if (c->scene_dirty) return build_scene_local(c);
        if (c->xf_dirty || local_scene_magnitude(c) > c->bvh.magnitude) { int r = run_geometry_kernels(c, true); if (r) return r; c->xf_dirty = false; }
        return 0;
    }
    if (c->scene_dirty) return build_scene(c);
    if (c->deform_pending) { int r = deform_update(c); if (r) return r; }
    const float om = std::max(camera_magnitude(c->params), c->sphere_mag);
    return om > c->bvh.magnitude ? repad_boxes(c, 2.0f * om) : 0;     // widen the box padding, keep the tree
}

// After prepare_scene: ray origins of a query reach |coordinate| G.  The rule prepare_scene applies to the camera: world-space uploads
// widen the padding to twice G, local ones run the geometry pass with G.  (Twice a finite G above FLT_MAX / 2 is FLT_MAX, not +inf: a pad
// of +inf would turn the empty child slots' (+inf, -inf) boxes into NaN ones; FLT_MAX still bounds every finite origin.)
int cover_origins(rt_ctx* c, float G)
{
    if (!(G > c->bvh.magnitude)) return 0;
    return c->geom_local ? run_geometry_kernels(c, true, G) : repad_boxes(c, std::min(2.0f * G, FLT_MAX));
}

// Give `dst` the scene `src` has built (world-space uploads): every device buffer is copied device to device — over xGMI when the
// contexts sit on different GPUs — and the host-side description of the tree comes along; dst builds nothing and holds no host copy of
// the triangles.  rt_multi uses it so that N contexts cost one BVH build and one host -> device upload per scene change.
template <class T> int clone_buf(rt_ctx* dst, DevBuf<T>& d, const rt_ctx* src, const DevBuf<T>& s)
{
    RT_HIP(dst, d.ensure(s.used));
    if (!s.used) return 0;
    if (dst->device == src->device && !dst->opt_peer_copies) RT_HIP(dst, hipMemcpyAsync(d.p, s.p, s.used * sizeof(T), hipMemcpyDeviceToDevice, dst->stream));
    else RT_HIP(dst, hipMemcpyPeerAsync(d.p, dst->device, s.p, src->device, s.used * sizeof(T), dst->stream));
    return 0;
}
int clone_scene(rt_ctx* dst, rt_ctx* src)
{
    if (src->scene_dirty || src->geom_local) return fail(dst, -2, "clone_scene: the source context has no built world-space scene");
    RT_HIP(dst, hipSetDevice(src->device));
    RT_HIP(dst, hipStreamSynchronize(src->stream));
    RT_HIP(dst, hipSetDevice(dst->device));
#define RT_CLONE(B) { int r_ = clone_buf(dst, dst->B, src, src->B); if (r_) return r_; }
    RT_CLONE(d_sph_geom) RT_CLONE(d_sph_mat) RT_CLONE(d_nodes) RT_CLONE(d_nodes_h) RT_CLONE(d_tri_geo) RT_CLONE(d_tri_nrm)
    RT_CLONE(d_chunk_mat) RT_CLONE(d_chunk_box) RT_CLONE(d_raw_tris) RT_CLONE(d_raw_range) RT_CLONE(d_order)
#undef RT_CLONE
    RT_HIP(dst, hipStreamSynchronize(dst->stream));
    dst->h_spheres.clear(); dst->h_tris.clear(); dst->h_mesh.clear(); dst->geom_local = false;
    dst->tris_resident = false; dst->n_resident = 0; dst->tree_resident = false; dst->deform_pending = false;   // (a received scene is nobody's upload)
    dst->bvh.nodes.clear(); dst->bvh.order.clear();
    dst->bvh.levelStart = src->bvh.levelStart; dst->bvh.maxStack = src->bvh.maxStack; dst->bvh.depth = src->bvh.depth; dst->bvh.magnitude = src->bvh.magnitude;
    dst->n_nodes = src->n_nodes; dst->area_at_build = src->area_at_build;
    dst->n_spheres = src->n_spheres; dst->n_tris = src->n_tris; dst->n_chunks = src->n_chunks; dst->sphere_mag = src->sphere_mag;
    dst->stats.numSpheres = src->stats.numSpheres; dst->stats.numTriangles = src->stats.numTriangles; dst->stats.numMeshChunks = src->stats.numMeshChunks;
    dst->stats.numBvhNodes = src->stats.numBvhNodes; dst->stats.bvhMaxStack = src->stats.bvhMaxStack; dst->stats.bvhInternalArea = src->stats.bvhInternalArea;
    dst->stats.bvhBuiltOnDevice = src->stats.bvhBuiltOnDevice; dst->stats.lastBvhBuildMs = 0.0;
    dst->scene_dirty = false; dst->tile_order_valid = false; dst->auto_choice = -1; dst->scene_version++;
    return 0;
}

// The rows this context renders (rt_set_rows / rt_set_bands) of the image of c->params
int strip_layout(rt_ctx* c, StripLayout& L)
{
    const int H = c->params.height;
    L.w = c->params.width; L.h = H;
    L.row0 = c->nrows < 0 ? 0 : c->row0; L.rows = c->nrows < 0 ? H : c->nrows; L.row_stride = 8;
    if (c->band_stride > 0) {
        // bands band_first, band_first + band_stride, ... of 8 rows each; the image's last band may be partial
        L.row0 = c->band_first * 8; L.row_stride = c->band_stride * 8; L.rows = 0;
        for (int y = L.row0; y < H; y += L.row_stride) L.rows += std::min(8, H - y);
        if (L.row0 > H) L.row0 = H;
    } else if (L.row0 < 0 || L.rows < 0 || L.row0 + L.rows > H) return fail(c, -6, "row strip [%d,%d) outside image height %d", L.row0, L.row0 + L.rows, H);
    return 0;
}

// `planes` are (re)created for the layout L, cleared: a re-created render texture starts cleared (ShaderHelper.CreateRenderTexture,
// ShaderHelper.cs:186-205)
int create_planes(rt_ctx* c, const StripLayout& L, std::initializer_list<DevBuf<float4>*> planes)
{
    const size_t px = L.pixels();
    for (DevBuf<float4>* b : planes) {
        RT_HIP(c, b->ensure(px));
        if (px) RT_HIP(c, hipMemsetAsync(b->p, 0, px * sizeof(float4), c->stream));
    }
    return 0;
}

int ensure_targets(rt_ctx* c)
{
    StripLayout L;
    { int r = strip_layout(c, L); if (r) return r; }
    if (L == c->target) return 0;           // (a context that never rendered holds the layout of an empty image)
    { int r = create_planes(c, L, { &c->d_frame, &c->d_accum }); if (r) return r; }
    c->target = L; c->tile_order_valid = false;
    c->stats.numRenderedFrames = 0; c->stats.totalKernelMs = 0;
    return 0;
}

enum class Variant { Fast, Counting, Flat };

// The camera fields of rt_params (viewParams, camLocalToWorld, worldSpaceCameraPos: what UpdateCameraParams sets, plus _WorldSpaceCameraPos)
// are one contiguous range; every other field is a setting.
constexpr size_t kCamBegin = offsetof(rt_params, viewParams), kCamEnd = offsetof(rt_params, worldSpaceLightPos0);
static_assert(offsetof(rt_params, camLocalToWorld) == kCamBegin + 12 && offsetof(rt_params, worldSpaceCameraPos) == kCamBegin + 76
              && kCamEnd == kCamBegin + 88, "the camera fields of rt_params are contiguous");
bool same_settings(const rt_params& a, const rt_params& b)
{
    return std::memcmp(&a, &b, kCamBegin) == 0 && std::memcmp((const char*)&a + kCamEnd, (const char*)&b + kCamEnd, sizeof(rt_params) - kCamEnd) == 0;
}
// the first entry of params[0 .. n - 1] whose settings differ from entry 0's, 0 if none does (rt_render_params, rt_multi_render_params)
int other_settings(const rt_params* params, int n)
{
    for (int f = 1; f < n; ++f) if (!same_settings(params[f], params[0])) return f;
    return 0;
}
// p (same settings as c->params) becomes the context's params, as rt_set_params(p) would make it
void use_camera(rt_ctx* c, const rt_params& p)
{
    if (std::memcmp(&c->params, &p, sizeof p) != 0) c->tile_order_stale = true;
    c->params = p;
}

// the per-launch figures of rt_stats summed over the launches of one call
void add_launch_stats(rt_stats& sum, const rt_stats& s)
{
    sum.rays += s.rays; sum.sphereTests += s.sphereTests; sum.nodeVisits += s.nodeVisits; sum.triTests += s.triTests; sum.hits += s.hits;
    for (int k = 0; k < 5; ++k) { sum.phaseLanes[k] += s.phaseLanes[k]; sum.phaseExecs[k] += s.phaseExecs[k]; }
    for (int k = 0; k < rtk::kNumRegions; ++k) sum.regionExecs[k] += s.regionExecs[k];
    sum.lastKernelMs += s.lastKernelMs;
}
void set_launch_stats(rt_stats& st, const rt_stats& sum)
{
    st.rays = sum.rays; st.sphereTests = sum.sphereTests; st.nodeVisits = sum.nodeVisits; st.triTests = sum.triTests; st.hits = sum.hits;
    for (int k = 0; k < 5; ++k) { st.phaseLanes[k] = sum.phaseLanes[k]; st.phaseExecs[k] = sum.phaseExecs[k]; }
    for (int k = 0; k < rtk::kNumRegions; ++k) st.regionExecs[k] = sum.regionExecs[k];
    st.lastKernelMs = sum.lastKernelMs;
}

// f(std::bool_constant<a>, std::bool_constant<b>, std::bool_constant<c>) for run-time a, b, c
template <class Fn> const void* dispatch3(bool a, bool b, bool c3, Fn f)
{
    auto lvl2 = [&](auto A) {
        auto lvl3 = [&](auto B) { return c3 ? f(A, B, std::true_type{}) : f(A, B, std::false_type{}); };
        return b ? lvl3(std::true_type{}) : lvl3(std::false_type{});
    };
    return a ? lvl2(std::true_type{}) : lvl2(std::false_type{});
}

// What a launch_frames_k call launches, and with which arguments
struct LaunchPlan {
    rtk::DeviceScene S{}; rtk::FrameArgs F{}; rtk::StreamArgs A{};
    const void* fn = nullptr; size_t lds = 0;
    int grid = 1, batch = 1, ntiles = 0, sample_lanes_log2 = 0;
    bool philox = false, stream = false, tile_kernel = false, stream_sync = false, cam_table = false, record_costs = false;
};

// The device scene every kernel reads
int fill_scene(rt_ctx* c, rtk::DeviceScene& S)
{
    S.sph_geom = c->d_sph_geom.p; S.sph_mat = c->d_sph_mat.p; S.nodes = c->d_nodes.p; S.nodes_h = c->d_nodes_h.p;
    S.tri_geo = c->d_tri_geo.p; S.tri_nrm = c->d_tri_nrm.p; S.chunk_mat = c->d_chunk_mat.p; S.chunk_box = c->d_chunk_box.p;
    S.raw_tris = c->d_raw_tris.p; S.raw_chunk_range = c->d_raw_range.p;
    S.ns = (int)c->n_spheres; S.nn = (int)c->n_nodes;
    // the kernels address nodes and BVH-order triangles with 32-bit byte offsets (128 B and 48 B records)
    if (c->n_nodes >= ((size_t)1 << 25) || c->n_tris >= ((size_t)1 << 32) / 48)
        return fail(c, -7, "scene too large for 32-bit record offsets (%zu BVH nodes)", c->n_nodes);
    S.nt = (int)c->n_tris;
    S.nm = (int)c->n_chunks;
    return 0;
}

// LDS traversal-stack entries per lane of the kernels that trace one query per lane to its end (k_trace, k_ray_query): the BVH's worst
// case, at most option "lds_stack", at most 64 — a very deep tree spills past 64 entries to the global overflow area instead of
// overflowing the LDS
int tile_stack_cap(const rt_ctx* c)
{
    int cap = std::max(1, c->bvh.maxStack);
    if (c->opt_lds_stack > 0) cap = std::min(cap, c->opt_lds_stack);
    return std::min(cap, 64);
}

// The traversal stack of a launch of such a kernel (k_trace, k_ray_query, k_aov) over `lanes` lanes: tile_stack_cap entries per lane in
// `lds` bytes of LDS per workgroup, and for a deeper tree the global overflow area — one slot per lane of the launch and entry beyond cap,
// so such a tree pays for the launch's width.  refuse_4g_for: the entry point whose launches are as wide as its image and that refuses
// an area above 4 GiB (null: the launch's width is bounded and the area is allocated whatever it takes)
struct LaneStack { int cap = 0; size_t lds = 0; uint32_t* gstack = nullptr; unsigned int stride = 0; };
int plan_lane_stack(rt_ctx* c, size_t lanes, LaneStack& st, const char* refuse_4g_for = nullptr)
{
    st.cap = tile_stack_cap(c);
    st.lds = (size_t)st.cap * 64 * sizeof(uint32_t) * rtk::kWavesPerBlock;
    static_assert(64 * 64 * sizeof(uint32_t) * rtk::kWavesPerBlock <= 64 * 1024, "the largest cap needs no opt-in to more than 64 KiB of dynamic LDS");
    st.stride = (unsigned int)lanes; st.gstack = nullptr;
    if (c->bvh.maxStack > st.cap) {
        const size_t need = (size_t)(c->bvh.maxStack - st.cap) * lanes;
        if (refuse_4g_for && need > ((size_t)4 << 30) / sizeof(uint32_t))
            return fail(c, -7, "%s: the traversal-stack overflow area would take %zu MiB (raise option lds_stack)", refuse_4g_for, need >> 18);
        RT_HIP(c, c->d_gstack.ensure(need));
        st.gstack = c->d_gstack.p;
    }
    return 0;
}

// Kernel choice, traversal stack and LDS, grid, frames per launch, spill buffers (kernel: 0 k_trace, 1 k_stream)
int plan_launch(rt_ctx* c, Variant var, int kernel, const rt_params* cams, int n_frames, LaunchPlan& P)
{
    rtk::DeviceScene& S = P.S; rtk::FrameArgs& F = P.F; rtk::StreamArgs& A = P.A;
    { int r = fill_scene(c, S); if (r) return r; }

    F.p = c->params;
    F.row0 = c->target.row0; F.nrows = c->target.rows; F.row_stride = c->target.row_stride;
    F.tile_w_log2 = 3;
    F.tiles_x = (c->target.w + 7) / 8; F.tiles_y = (c->target.rows + 7) / 8;
    if (kernel == 0 && c->opt_tile_w_log2 != 3) {        // k_trace only: other tile shapes (same 64 pixels per wave)
        F.tile_w_log2 = c->opt_tile_w_log2;
        const int tw = 1 << F.tile_w_log2, th = 64 >> F.tile_w_log2;
        F.tiles_x = (c->target.w + tw - 1) / tw; F.tiles_y = (c->target.rows + th - 1) / th;
    }
    // the counter-based mode is k_stream's Philox instantiation whatever kernel was asked for (its estimator spreads a pixel's samples
    // over the lanes of a wave); NumRaysPerPixel < 1 draws nothing in either mode and goes to k_trace
    const bool philox = P.philox = c->params.rngMode == RT_RNG_PHILOX && c->params.numRaysPerPixel >= 1;
    if (philox && var == Variant::Flat) return fail(c, -2, "the flat validation kernel implements the PCG stream only");
    if (philox) kernel = 1;
    if (philox && (c->target.w > 65535 || c->target.rows > 65535)) return fail(c, -7, "the Philox mode addresses at most 65535 x 65535 pixels per context");
    if (philox && (c->params.numRaysPerPixel > 65000 || c->params.maxBounceCount > 32000))
        return fail(c, -7, "the Philox mode takes at most 65000 rays per pixel per frame and 32000 bounces (sample and bounce share one signed 32-bit register)");
    const bool stream = P.stream = kernel == 1 && var != Variant::Flat && c->params.numRaysPerPixel >= 1   // PCG or Philox instantiation
                                   && c->target.w <= 65535 && c->target.rows <= 65535                      // (16-bit pixel coordinates in k_stream's item tables)
                                   && c->params.numRaysPerPixel <= 65000 && c->params.maxBounceCount <= 32000;     // (sample and bounce share one register; beyond that PCG frames are k_trace's)
    const bool tile_kernel = P.tile_kernel = !stream && var != Variant::Flat;   // k_trace, PCG or Philox
    F.stack_cap = tile_kernel ? tile_stack_cap(c)
                              : std::max(1, c->bvh.maxStack) + (stream ? 3 : 0);    // the branch-free push writes up to 3 slots past the top
    // k_stream: at most opt_stream_stack entries per lane in LDS (30 = five workgroups per CU, 21 = seven); a deeper worst case spills
    const bool seven_waves = stream && !philox && var == Variant::Fast && c->opt_compact_nodes != 0 && c->n_nodes > 0;     // rt_stream.hpp stream_waves()
    const int stream_stack = c->opt_stream_stack > 0 ? c->opt_stream_stack : (seven_waves ? (RT_STREAM_WAVES >= 7 ? 21 : 24) : 30);
    const bool stream_spill = stream && F.stack_cap > stream_stack;
    if (stream_spill) F.stack_cap = stream_stack;
    F.full_sort = c->opt_full_sort;
    bool fixed_origin = camera_origin_is_fixed(c->params);
    if (cams) for (int f = 0; f < n_frames; ++f) fixed_origin = fixed_origin && camera_origin_is_fixed(cams[f]);      // (wave-uniform: all frames or none)
    F.fixed_origin = fixed_origin ? 1 : 0;
    F.out_frame = c->d_frame.p; F.accum = c->d_accum.p;
    F.tile_counter = c->d_tile_counter; F.counters = c->d_counters;

    const size_t lds = P.lds = var == Variant::Flat ? 0
                                       : (size_t)F.stack_cap * 64 * sizeof(uint32_t) * rtk::kWavesPerBlock
                                         + (stream ? (size_t)rtk::kGroupMax * sizeof(uint2) * rtk::kWavesPerBlock : 0);     // k_stream: + the groups' item tables
    if (lds > 160 * 1024) return fail(c, -7, "BVH needs a %d-entry traversal stack: exceeds the 160 KiB LDS", F.stack_cap);
    const bool counting = var == Variant::Counting;
    const bool compact = c->opt_compact_nodes != 0;            // k_trace / k_stream; the flat twin reads neither
    P.cam_table = cams != nullptr;
    const void* fn = P.fn = var == Variant::Flat ? (const void*)rtk::k_trace<false, true>
                   : stream ? (cams ? rtk::cam_stream_kernel(philox, compact, c->n_nodes > 0)
                                    : rtk::stream_kernel(counting, philox, compact, c->n_nodes > 0))     // instantiated in rt_stream_kernels.hip
                   : c->n_nodes == 0      // spheres only: the instantiation compiled for six waves per SIMD
                            ? dispatch3(counting, false, false, [](auto C, auto, auto) { return (const void*)rtk::k_trace<decltype(C)::value, false, false, 6>; })
                            : dispatch3(counting, false, compact, [](auto C, auto, auto H) { return (const void*)rtk::k_trace<decltype(C)::value, false, decltype(H)::value>; });
    if (lds > 64 * 1024) RT_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int per_cu = 0;
    RT_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, rtk::kBlock, lds));
    if (per_cu < 1) return fail(c, -7, "kernel does not fit a CU (LDS %zu B)", lds);
    P.ntiles = F.tiles_x * F.tiles_y;
    // work items of a multi-frame launch = tiles x frames: a thin strip (one rank of eight: 4,080 tiles) still fills every resident wave
    // Philox mode: S = 16 / 4 / 1 sample lanes per pixel (the estimator's sub-streams, include/rt.h RT_RNG_PHILOX)
    P.sample_lanes_log2 = !philox ? 0 : c->params.numRaysPerPixel >= 16 ? 4 : c->params.numRaysPerPixel >= 4 ? 2 : 0;
    const bool stream_sync = P.stream_sync = stream && (c->opt_tile_sync || philox);       // k_stream taking whole work items (the Philox instantiation always does)
    if (cams && !stream_sync) return fail(c, -7, "per-frame cameras: no k_cam_stream launch for this target");
    const size_t frames_in_queue = ((stream_sync && c->opt_frame_batch != 1) ? (size_t)std::max(1, std::min(n_frames, 64)) : 1) << P.sample_lanes_log2;
    const int want = (int)std::min<size_t>(((size_t)P.ntiles * frames_in_queue + rtk::kWavesPerBlock - 1) / rtk::kWavesPerBlock, (size_t)1 << 20);
    if (c->opt_blocks_per_cu > 0) per_cu = std::min(per_cu, c->opt_blocks_per_cu);
    const int grid = P.grid = std::max(1, std::min(want, per_cu * c->n_cu));
    A.shade_threshold = std::max(1, std::min(64, c->opt_shade_threshold));
    A.total_pixels = (unsigned int)P.ntiles * 64u;
    A.tile_sync = stream_sync ? 1 : 0;
    A.sample_lanes_log2 = P.sample_lanes_log2;
    A.tiles_per_fetch = std::max(1, std::min(rtk::kGroupMax, c->opt_tiles_per_fetch));
    A.guide_div = 1;
    A.node_min = std::max(1, std::min(64, c->opt_node_min));
    const unsigned int gstack_stride = (unsigned int)grid * rtk::kBlock;
    if (philox) {      // where the lanes park their sub-stream sums until the wave's group of items is done: [wave][item of the group][3][64]
        RT_HIP(c, c->d_park.ensure((size_t)grid * rtk::kWavesPerBlock * (size_t)A.tiles_per_fetch * 192));
        F.park = c->d_park.p;
    }
    if (stream_spill) {
        RT_HIP(c, c->d_gstack.ensure((size_t)(c->bvh.maxStack + 3 - F.stack_cap) * gstack_stride));
        F.gstack = c->d_gstack.p; F.gstack_stride = gstack_stride;
    }
    if (tile_kernel) {
        LaneStack st;
        { int r = plan_lane_stack(c, gstack_stride, st); if (r) return r; }
        F.gstack = st.gstack; F.gstack_stride = st.gstack ? st.stride : 0;
    }
    // k_trace can trace several frames per launch (work items = (frame, tile)): the persistent waves then balance over
    // frames as well — what matters when a rank's strip has about as many tiles as the chip has wave slots.
    // k_stream taking whole tiles (stream_sync) has the same (frame, tile) items as k_trace
    if ((tile_kernel || stream_sync) && n_frames > 1 && c->opt_frame_batch != 1) {
        const size_t budget = (size_t)4 << 30;                                  // <= 4 GiB of per-frame outputs (16 frames at 3840x2160)
        const size_t per_frame = c->target.pixels() * sizeof(float4);
        int batch = (int)std::min<size_t>((size_t)n_frames, std::max<size_t>(1, budget / per_frame));
        if (c->opt_frame_batch > 1) batch = std::min(batch, c->opt_frame_batch);
        P.batch = batch = std::min(batch, 256);
        if (batch > 1) RT_HIP(c, c->d_batch.ensure((size_t)batch * c->target.pixels()));
    }
    return 0;
}

// LPT scheduling of the persistent waves: a launch records every tile's cost; the next ones hand tiles out costliest
// first, so the end of a launch is filled with cheap tiles instead of waiting for a few expensive ones.
int plan_tile_order(rt_ctx* c, LaunchPlan& P)
{
    const int ntiles = P.ntiles;
    const bool lpt = (P.tile_kernel || P.stream_sync) && c->opt_tile_lpt && ntiles > 1;
    c->lpt_active = lpt;
    if (!lpt) return 0;
    if (c->tile_order_n != ntiles) { c->tile_order_valid = false; c->tile_order_n = ntiles; }
    RT_HIP(c, c->d_tile_cost.ensure(ntiles)); RT_HIP(c, c->d_tile_order.ensure(ntiles));
    if (!c->tile_order_valid || c->tile_order_stale) {
        P.record_costs = true;
        RT_HIP(c, hipMemsetAsync(c->d_tile_cost.p, 0, (size_t)ntiles * sizeof(uint32_t), c->stream));
    }
    P.F.tile_order = c->tile_order_valid ? c->d_tile_order.p : nullptr;
    P.F.tile_cost = P.record_costs ? c->d_tile_cost.p : nullptr;
    return 0;
}

// Camera rays' candidate lists: every pixel's camera rays start from <= 4 leaves found once per camera / scene (rt_primary.hpp)
int ensure_primary_lists(rt_ctx* c, LaunchPlan& P)
{
    const bool eligible = P.stream && !P.cam_table && c->opt_primary_lists && c->n_nodes > 0 && P.F.fixed_origin && c->target.pixels() > 0
                          && c->bvh.maxStack <= 160;
    if (!eligible) return 0;
    std::string key((const char*)&c->params, sizeof c->params);
    const unsigned long long geo[6] = { c->scene_version, (unsigned long long)c->target.row0, (unsigned long long)c->target.rows,
                                        (unsigned long long)c->target.row_stride, (unsigned long long)c->target.w, (unsigned long long)c->target.h };
    key.append((const char*)geo, sizeof geo);
    if (key != c->primary_key) {     // (the build takes well under a millisecond at 1080p: a camera that moves every frame pays it every frame and still gains)
        RT_HIP(c, c->d_primary.ensure(c->target.pixels())); RT_HIP(c, c->d_focus.ensure(c->target.pixels())); RT_HIP(c, c->d_primary_counts.ensure(4));
        RT_HIP(c, hipMemsetAsync(c->d_primary_counts.p, 0, 4 * sizeof(unsigned int), c->stream));
        rtp::PrimaryArgs PA{};
        PA.p = c->params; PA.row0 = c->target.row0; PA.nrows = c->target.rows; PA.row_stride = c->target.row_stride;
        PA.lists = c->d_primary.p; PA.focus = c->d_focus.p; PA.counts = c->d_primary_counts.p;
        const int tiles = ((c->target.w + 7) / 8) * ((c->target.rows + 7) / 8);
        PA.stack_cap = std::max(1, c->bvh.maxStack);                       // (the whole worst case in LDS: at most 160 entries x 64 lanes x 4 B = 40 KB per wave)
        const size_t plds = (size_t)PA.stack_cap * 64 * sizeof(uint32_t);
        RT_HIP(c, hipEventRecord(c->evg0, c->stream));
        hipLaunchKernelGGL(rtp::k_primary_lists, dim3(tiles), dim3(64), plds, c->stream, P.S, PA);
        RT_HIP(c, hipGetLastError());
        RT_HIP(c, hipEventRecord(c->evg1, c->stream));
        unsigned int h[4];
        RT_HIP(c, hipMemcpyAsync(h, c->d_primary_counts.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        RT_HIP(c, hipEventElapsedTime(&ms, c->evg0, c->evg1));
        for (int k = 0; k < 4; ++k) c->stats.primaryLists[k] = h[k];
        c->stats.lastPrimaryListsMs = ms; c->stats.primaryListBuilds++;
        c->primary_key = key;
    }
    P.F.primary = c->d_primary.p; P.F.focus = c->d_focus.p;
    return 0;
}

// Per-frame cameras: the launch's camera table (a launch of frames i .. i + nb - 1 reads its records from entry i)
int upload_camera_table(rt_ctx* c, const rt_params* cams, int n_frames)
{
    c->h_cams.resize((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const rt_params& q = cams[f];
        rtk::CamRecord& rec = c->h_cams[f];
        rec.view = make_float4(q.viewParams[0], q.viewParams[1], q.viewParams[2], 0.f);
        rec.m0 = f4(q.camLocalToWorld); rec.m1 = f4(q.camLocalToWorld + 4); rec.m2 = f4(q.camLocalToWorld + 8);
        rec.pos = make_float4(q.worldSpaceCameraPos[0], q.worldSpaceCameraPos[1], q.worldSpaceCameraPos[2], 0.f);
    }
    RT_HIP(c, upload(c, c->d_cams, c->h_cams));
    return 0;
}

// The trace launches of frames first_frame .. first_frame + n_frames - 1, P.batch frames per launch, each batch accumulated
int run_launches(rt_ctx* c, LaunchPlan& P, int first_frame, int n_frames)
{
    rtk::FrameArgs& F = P.F; rtk::StreamArgs& A = P.A;
    RT_HIP(c, hipMemsetAsync(c->d_counters, 0, rtk::kNumCounters * sizeof(unsigned long long), c->stream));
    RT_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < n_frames; ) {
        int nb = P.batch > 1 ? std::min(P.batch, n_frames - i) : 1;
        // k_stream, frame-interleaved sub-tiles: a wave = (4x4 or 2x2 pixels) x (4 or 16 frames); launches take whole frame
        // groups, the remainder of the render goes out as 8x8 x 1 items
        A.n16 = A.n4 = 0; A.n1 = nb;
        if (P.stream_sync) {
            // as many groups of 16 frames as fit, then groups of 4, the rest one by one — all in this one launch
            int rem = nb;
            if (!P.philox && c->opt_stream_tile >= 4) { A.n16 = rem / 16; rem -= A.n16 * 16; }      // (Philox: sample lanes, not frames, fill a wave)
            if (!P.philox && c->opt_stream_tile >= 2) { A.n4 = rem / 4; rem -= A.n4 * 4; }
            A.n1 = rem;
            // groups shrink towards the end of the launch (k_stream: guided self-scheduling): up to tiles_per_fetch items per fetch
            // while more than guide x (waves of the launch) x that many items are left
            A.tiles_per_fetch = std::max(1, std::min(rtk::kGroupMax, c->opt_tiles_per_fetch));
            // (Philox: the units of a group are small — a few samples — and handed out dynamically, so big groups balance by themselves and
            // only the launch's last round of groups needs to shrink: a single 1080p frame 19.2 -> 17.5 ms with guide 1; PCG units are whole
            // pixels and need the finer tail: 19.9 -> 47.9 ms with it)
            A.guide_div = std::max(1, P.grid * rtk::kWavesPerBlock * (P.philox ? std::max(1, c->opt_fetch_guide_philox) : std::max(1, c->opt_fetch_guide)));
        }
        F.frame = first_frame + i;
        F.frames_in_launch = nb; F.frame_stride = (unsigned int)c->target.pixels();
        F.out_frame = nb > 1 ? c->d_batch.p : c->d_frame.p;
        RT_HIP(c, hipMemsetAsync(c->d_tile_counter, 0, sizeof(unsigned int), c->stream));
        {
            const rtk::CamRecord* cam_tab = P.cam_table ? c->d_cams.p + i : nullptr;
            void* args[4] = { (void*)&P.S, (void*)&F, (void*)&A, (void*)&cam_tab };    // k_trace takes (S, F) only, k_stream (S, F, A)
            RT_HIP(c, hipLaunchKernel(P.fn, dim3(P.grid), dim3(rtk::kBlock), args, P.lds, c->stream));
        }
        RT_HIP(c, hipGetLastError());
        if (nb > 1) {
            const int ag = (int)std::min<size_t>((c->target.pixels() + 255) / 256, (size_t)c->n_cu * 8);
            hipLaunchKernelGGL(rtk::k_accumulate<>, dim3(ag), dim3(256), 0, c->stream, c->d_batch.p, c->d_accum.p, c->d_frame.p,
                               c->target.pixels(), F.frame_stride, F.frame, nb);
            RT_HIP(c, hipGetLastError());
        }
        i += nb;
    }
    return 0;
}

// After the launches: the kernel time, the tile order for the next launches and the counters
int finish_launch(rt_ctx* c, const LaunchPlan& P, Variant var, int n_frames)
{
    c->stats.lastFramesPerLaunch = P.batch;
    c->stats.lastKernel = var == Variant::Flat ? 4 : P.stream ? (P.cam_table ? 2 : 1) : 0;
    c->stats.lastFramesInterleaved = P.stream ? (P.philox ? 1 : P.A.n16 ? 16 : P.A.n4 ? 4 : 1) : 1;
    c->stats.lastSampleLanes = P.philox ? 1 << P.sample_lanes_log2 : 1;
    RT_HIP(c, hipEventRecord(c->ev1, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.lastKernelMs = ms; c->stats.totalKernelMs += ms;
    if (P.record_costs) {
        // costliest tiles first for the next launches: counting sort on the device, no host round trip
        const uint32_t ntiles = (uint32_t)P.ntiles;
        RT_HIP(c, c->d_tile_hist.ensure(rtg::kCostBuckets));
        RT_HIP(c, hipMemsetAsync(c->d_tile_hist.p, 0, rtg::kCostBuckets * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(rtg::k_tile_hist, dim3((ntiles + 255) / 256), dim3(256), 0, c->stream, c->d_tile_cost.p, ntiles, c->d_tile_hist.p);
        hipLaunchKernelGGL(rtg::k_tile_scan, dim3(1), dim3(1024), 0, c->stream, c->d_tile_hist.p);
        hipLaunchKernelGGL(rtg::k_tile_scatter, dim3((ntiles + 255) / 256), dim3(256), 0, c->stream, c->d_tile_cost.p, ntiles,
                           c->d_tile_hist.p, c->d_tile_order.p);
        RT_HIP(c, hipGetLastError());
        c->tile_order_valid = true; c->tile_order_stale = false;
    }
    c->stats.numRenderedFrames += n_frames;
    unsigned long long h[rtk::kNumCounters];
    RT_HIP(c, hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    c->stats.rays = h[0];                        // counted by every variant
    const bool counting = var == Variant::Counting;
    c->stats.sphereTests = counting ? h[1] : 0; c->stats.nodeVisits = counting ? h[2] : 0; c->stats.triTests = counting ? h[3] : 0; c->stats.hits = counting ? h[4] : 0;
    for (int k = 0; k < 5; ++k) { c->stats.phaseLanes[k] = counting ? h[5 + k] : 0; c->stats.phaseExecs[k] = counting ? h[10 + k] : 0; }
    for (int k = 0; k < rtk::kNumRegions; ++k) c->stats.regionExecs[k] = counting ? h[15 + k] : 0;
    return 0;
}

// One kernel choice for all n_frames (kernel: 0 k_trace, 1 k_stream).
// cams: frame first_frame + f has the uniforms cams[f] (rt_render_params; all with the settings of c->params); null = c->params for all.
int launch_frames_k(rt_ctx* c, int first_frame, int n_frames, Variant var, int kernel, const rt_params* cams = nullptr)
{
    if (!c) return -1;
    if (!c->have_params) return fail(c, -2, "rt_set_params has not been called");
    if (n_frames < 0) return fail(c, -2, "n_frames < 0");
    if (n_frames == 0) cams = nullptr;
    // Per-frame cameras.  A k_stream launch of several frames becomes a k_cam_stream launch with a camera table (one record per frame);
    // every other launch — one frame, k_trace, the counting build, the flat twin — goes frame by frame with the frame's camera in
    // c->params.  Both give the bits of the per-frame loop rt_set_params + rt_render_frame.
    const bool philox = c->params.rngMode == RT_RNG_PHILOX && c->params.numRaysPerPixel >= 1;
    const bool table = n_frames > 1 && var == Variant::Fast && (kernel == 1 || philox) && c->params.numRaysPerPixel >= 1
                       && (c->opt_tile_sync || philox) && c->params.width <= 65535 && c->params.height <= 65535;     // (= stream_sync of plan_launch)
    if (cams && !table) {
        rt_stats sum{};
        for (int f = 0; f < n_frames; ++f) {
            use_camera(c, cams[f]);
            const int r = launch_frames_k(c, first_frame + f, 1, var, kernel);
            if (r) return r;
            add_launch_stats(sum, c->stats);
        }
        set_launch_stats(c->stats, sum);
        return 0;
    }
    if (cams) {     // the box padding (prepare_scene, from c->params) for the camera that reaches farthest
        int far = 0;
        for (int f = 1; f < n_frames; ++f) if (camera_magnitude(cams[f]) > camera_magnitude(cams[far])) far = f;
        use_camera(c, cams[far]);
    }
    c->frames_traced += (uint64_t)n_frames;     // (before the build: the moving-scene window of build_scene counts this launch)
    RT_HIP(c, hipSetDevice(c->device));
    { int r = prepare_scene(c); if (r) return r; }
    if (cams) use_camera(c, cams[n_frames - 1]);      // (from here on only the settings of c->params are read; the context ends with the last frame's)
    { int r = ensure_targets(c); if (r) return r; }
    if (c->target.pixels() == 0 || n_frames == 0) return 0;
    LaunchPlan P;
    int r = plan_launch(c, var, kernel, cams, n_frames, P);
    if (!r) r = plan_tile_order(c, P);
    if (!r) r = ensure_primary_lists(c, P);
    if (!r && cams) r = upload_camera_table(c, cams, n_frames);
    if (!r) r = run_launches(c, P, first_frame, n_frames);
    return r ? r : finish_launch(c, P, var, n_frames);
}

// Kernel choice "auto" (option kernel = -1, the default): k_trace and k_stream (resumable traversal, stragglers deferred)
// produce the same bits, and which one is faster depends on the scene (measured: k_stream +8 % on the 100k-triangle
// workload, -5 % on the 1M-triangle one, -13 % on spheres only).  So the first frames after a scene / camera change are
// used as the measurement: one frame records the tile costs, one is timed with k_trace, one with k_stream (all three are
// ordinary frames of the render — nothing is traced twice); the faster kernel takes the rest.
int launch_frames(rt_ctx* c, int first_frame, int n_frames, Variant var, const rt_params* cams = nullptr)
{
    if (!c) return -1;
    const bool eligible = c->opt_kernel < 0 && var != Variant::Flat && c->have_params
                          && c->params.numRaysPerPixel >= 1 && c->params.rngMode != RT_RNG_PHILOX;   // (Philox: always k_stream)
    if (!eligible) {
        const int kernel = c->opt_kernel < 0 ? 0 : c->opt_kernel;
        return launch_frames_k(c, first_frame, n_frames, var, kernel, cams);
    }
    // (with the costliest-first order switched off, or a single tile, there is no order to wait for)
    auto order_ready = [&]() { return c->tile_order_valid || !c->lpt_active; };
    // Decided: single frames go to the kernel that won the single-frame timing; launches of 4 frames or more over a BVH go to
    // k_stream, whose frame-interleaved items (2x2 pixels x 16 frames per wave) have no counterpart in k_trace (measured on both
    // triangle workloads: +13 % / +10 % over its own 8x8 x 1 items, which is what the single-frame timing compares)
    auto decided = [&](int frames) { return (c->stats.numBvhNodes > 0 && frames >= 4 && c->opt_tile_sync) ? 1 : c->auto_choice; };
    if (c->auto_choice >= 0 && !c->scene_dirty && order_ready())
        return launch_frames_k(c, first_frame, n_frames, var, decided(n_frames), cams);

    if (n_frames == 0) {            // scene / geometry update only (rt_multi's build on its first context)
        const bool was_dirty = c->scene_dirty;
        const int r = launch_frames_k(c, first_frame, 0, var, c->auto_choice >= 0 ? c->auto_choice : 0);
        if (was_dirty) { c->auto_choice = -1; c->auto_ms[0] = c->auto_ms[1] = -1.0; }     // a new scene is measured again, as on the contexts that receive it
        return r;
    }
    rt_stats sum{}; bool any = false;
    auto add = [&]() { add_launch_stats(sum, c->stats); any = true; };
    int done = 0;
    while (done < n_frames) {
        int kernel, count = 1;
        if (c->scene_dirty || !order_ready()) { kernel = 0; c->auto_choice = -1; c->auto_ms[0] = c->auto_ms[1] = -1.0; }   // records the tile costs
        else if (c->auto_choice >= 0) { count = n_frames - done; kernel = decided(count); }
        else if (c->auto_ms[0] < 0) kernel = 0;
        else kernel = 1;
        const bool probing = c->auto_choice < 0 && !c->scene_dirty && order_ready();
        int r = launch_frames_k(c, first_frame + done, count, var, kernel, cams ? cams + done : nullptr);
        if (r) return r;
        add();
        if (c->target.pixels() == 0) { done += count; continue; }
        // a kernel variant's very first launch in a context also pays its one-off set-up (code upload, the scratch ring of
        // k_stream): that frame is rendered like any other but not used as the timing
        const int variant = kernel * 4 + (c->params.rngMode == RT_RNG_PHILOX ? 2 : 0) + (c->opt_compact_nodes ? 1 : 0);
        const bool first_use = !((c->variants_launched >> variant) & 1u);
        c->variants_launched |= 1u << variant;
        if (probing) {
            if (!first_use) c->auto_ms[kernel] = c->stats.lastKernelMs;
            if (c->auto_ms[0] >= 0 && c->auto_ms[1] >= 0) c->auto_choice = (c->stats.numBvhNodes > 0 && c->auto_ms[1] < c->auto_ms[0]) ? 1 : 0;
        }
        done += count;
    }
    if (any) set_launch_stats(c->stats, sum);
    c->stats.autoKernel = c->auto_choice;
    return 0;
}

// The end of every read of a plane: n_floats must be the plane's expect_floats (`shape`: what the message calls that product), then one
// copy on the stream of `on` — the context that holds the plane: o itself, or the first context of the handle o — waited for.  What a
// null destination means is the entry point's own rule, checked before.
int copy_plane(ErrOwner* o, const rt_ctx* on, const void* src, size_t expect_floats, const char* shape, void* dst, size_t n_floats, bool to_device)
{
    if (n_floats != expect_floats) return fail(o, -2, "expected %zu floats (%s), got %zu", expect_floats, shape, n_floats);
    if (!n_floats) return 0;
    RT_HIP(o, hipSetDevice(on->device));
    RT_HIP(o, hipMemcpyAsync(dst, src, n_floats * sizeof(float), to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, on->stream));
    RT_HIP(o, hipStreamSynchronize(on->stream));
    return 0;
}

int read_target(rt_ctx* c, bool accum, float* dst, size_t n_floats, bool to_device)
{
    if (!c) return -1;
    if (!dst && n_floats) return fail(c, -2, "null destination");
    if (c->have_params) { int r = ensure_targets(c); if (r) return r; }
    return copy_plane(c, c, accum ? c->d_accum.p : c->d_frame.p, c->target.pixels() * 4, "rows*width*4", dst, n_floats, to_device);
}

// Frames first .. first + n - 1 with the uniforms params[f] (all with the settings of c->params).  One camera for all: today's path
// (candidate lists, cached focus points, k_stream) — a static camera pays nothing for the per-frame form.  Otherwise k_cam_stream's
// camera table (launch_frames_k).  The context ends with params[n - 1].
int launch_run(rt_ctx* c, int first, int n, const rt_params* params)
{
    bool one_camera = true;
    for (int f = 1; f < n && one_camera; ++f) one_camera = std::memcmp(&params[f], &params[0], sizeof(rt_params)) == 0;
    if (one_camera) { use_camera(c, params[0]); return launch_frames(c, first, n, Variant::Fast); }
    return launch_frames(c, first, n, Variant::Fast, params);
}

// ---- queued submission ----------------------------------------------------------------------------------------------------------
void queue_worker(rt_ctx* c)
{
    std::unique_lock<std::mutex> lk(c->q_mu);
    std::vector<rt_params> run;
    for (;;) {
        c->q_cv.wait(lk, [&] { return c->q_stop || !c->q_frames.empty(); });
        if (c->q_frames.empty()) break;                 // (stop is honoured once the queue has drained)
        if (c->opt_queue_linger_us > 0 && !c->q_stop)
            c->q_cv.wait_for(lk, std::chrono::microseconds(c->opt_queue_linger_us), [&] { return c->q_stop || (int)c->q_frames.size() >= c->opt_queue_depth; });
        // the longest run of consecutive frame indices at the head of the queue: one launch (rt_render(first, n))
        // (its frames share the settings — a change of settings settles the queue before it is queued — and may differ in camera)
        const int first = c->q_frames.front().frame; int n = 0;
        run.clear();
        while (!c->q_frames.empty() && c->q_frames.front().frame == first + n && n < c->opt_queue_depth) { run.push_back(c->q_frames.front().p); c->q_frames.pop_front(); ++n; }
        c->q_busy = true;
        const bool failed = c->q_rc != 0;
        lk.unlock();
        const int r = failed ? 0 : launch_run(c, first, n, run.data());      // after a failure the rest of the queue is dropped
        lk.lock();
        if (r && !c->q_rc) { c->q_rc = r; c->q_err = c->err; }
        if (!failed && !r) c->stats.queuedLaunches++;
        c->q_busy = false;
        c->q_idle.notify_all();
    }
}

// Every entry point but rt_submit_frame starts here: the queue is empty and the worker idle before anything else touches the context
// (a context has one caller thread; the worker is the library's own).  Returns the first error a queued launch met, once.
int settle(rt_ctx* c)
{
    if (!c->q_started) return 0;
    std::unique_lock<std::mutex> lk(c->q_mu);
    c->q_idle.wait(lk, [&] { return c->q_frames.empty() && !c->q_busy; });
    const int r = c->q_rc;
    if (r) { c->err = "queued frame: " + c->q_err; c->q_rc = 0; }
    return r;
}
#define RT_SETTLE(c) do { const int qr_ = settle(c); if (qr_) return qr_; } while (0)

// (with c->q_mu held) queue frame `frame` with the uniforms p; the worker starts with the first frame
void queue_push(rt_ctx* c, int frame, const rt_params& p)
{
    if (!c->q_started) { c->q_thread = std::thread(queue_worker, c); c->q_started = true; }
    c->q_frames.push_back(rt_ctx::QItem{ frame, p });
    c->q_tail = p;
}
// (with c->q_mu held) the params the next queued frame follows: the last queued frame's, or the context's once the queue has run
// (the worker only changes c->params while it is busy)
const rt_params& queue_tail(const rt_ctx* c) { return (c->q_frames.empty() && !c->q_busy) ? c->params : c->q_tail; }

// ---- ray queries (rt_trace_rays / rt_occluded, csrc/rt_query.hpp) ---------------------------------------------------------------
constexpr int kQuerySlice = 1 << 22;    // rays per launch (and per staging slice of the host entries: 128 MiB of rays, 256 MiB of hits)

// Largest finite |origin coordinate| over the rays a query traces (tMax > 0)
float query_origin_bound(const rt_ray* rays, int n)
{
    float m = 0.f;
    for (int i = 0; i < n; ++i) {
        if (!(rays[i].tMax > 0.0f)) continue;
        for (int a = 0; a < 3; ++a) { const float v = std::fabs(rays[i].origin[a]); if (v > m && v <= 3.4028235e38f) m = v; }
    }
    return m;
}

// Settle, then make the scene current for rays whose origins reach |coordinate| G (host entries; the device entries measure G on the
// device between the two steps, query_prepare_device)
int query_prepare(rt_ctx* c, float G)
{
    RT_HIP(c, hipSetDevice(c->device));
    { int r = prepare_scene(c); if (r) return r; }
    return cover_origins(c, G);
}

// p lies in memory of the context's device (hipMalloc'ed or managed)
bool on_ctx_device(const rt_ctx* c, const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.isManaged) && a.device == c->device;
}

// the device in whose memory p lies (hipMalloc'ed or managed), -1: host memory (a plain host pointer makes the query fail)
int device_of_ptr(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.isManaged) ? a.device : -1;
}

// cover_origins for rays in device memory: the origin bound of the batch is measured on the device — one small kernel and a 4-byte
// read-back (the call's one synchronisation)
int cover_origins_device(rt_ctx* c, const float4* rays, int n)
{
    RT_HIP(c, c->d_q_bound.ensure(1));
    RT_HIP(c, hipMemsetAsync(c->d_q_bound.p, 0, sizeof(unsigned int), c->stream));
    const int grid = std::max(1, std::min((n + 255) / 256, 4 * std::max(1, c->n_cu)));
    hipLaunchKernelGGL(rtk::k_query_origin_bound<0>, dim3(grid), dim3(256), 0, c->stream, rays, n, c->d_q_bound.p);
    RT_HIP(c, hipGetLastError());
    unsigned int bits = 0;
    RT_HIP(c, hipMemcpyAsync(&bits, c->d_q_bound.p, sizeof bits, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return cover_origins(c, u2f(bits));
}

// ---- the one path of the six query families ----------------------------------------------------------------------------------------
// Ray queries (rt_trace_rays / rt_occluded, csrc/rt_query.hpp), radiance queries (rt_trace_radiance, csrc/rt_radiance.hpp), gather
// queries (rt_gather, csrc/rt_gather.hpp), visibility gathers (rt_visibility, csrc/rt_visibility.hpp), closest-point queries
// (rt_closest_points, csrc/rt_closest.hpp) and multi-hit ray queries (rt_trace_hits, csrc/rt_multihit.hpp) all take n rt_ray (2 float4 each) and write a fixed number of bytes per item.  A family supplies a description of the call (QueryCall, built by its *_call once
// the arguments are known to be good) and a function that fills its kernel's Args for one launch; everything between the exported
// entry and hipLaunchKernel is below, once.
enum QueryFamily { kRadiance, kGather, kVisibility, kClosest, kHits, kRays };    // (the first three: the sampled families; the first five are timed and index rt_ctx::query_info)

// The sampled families' params and info records have one layout: rt_radiance_* keeps reserved words where the other two have `mode`.
// rt_gather_params / rt_gather_info are the form the path works with.
#define RT_SAME_FIELD(A, B, a, b) static_assert(offsetof(A, a) == offsetof(B, b), #A "." #a " is not where " #B "." #b " is")
#define RT_SAME_PARAMS(T, mode_word) static_assert(sizeof(T) == sizeof(rt_gather_params), #T); RT_SAME_FIELD(T, rt_gather_params, samples, samples); \
    RT_SAME_FIELD(T, rt_gather_params, seed, seed); RT_SAME_FIELD(T, rt_gather_params, firstIndex, firstIndex); static_assert(offsetof(T, mode_word) == offsetof(rt_gather_params, mode), #T)
#define RT_SAME_INFO(T, mode_word) static_assert(sizeof(T) == sizeof(rt_gather_info), #T); RT_SAME_FIELD(T, rt_gather_info, samples, samples); \
    RT_SAME_FIELD(T, rt_gather_info, lastSampleLanes, lastSampleLanes); RT_SAME_FIELD(T, rt_gather_info, calls, calls); RT_SAME_FIELD(T, rt_gather_info, mode_word, mode); \
    RT_SAME_FIELD(T, rt_gather_info, lastKernelMs, lastKernelMs); RT_SAME_FIELD(T, rt_gather_info, totalKernelMs, totalKernelMs)
RT_SAME_PARAMS(rt_radiance_params, _reserved); RT_SAME_PARAMS(rt_visibility_params, mode);
RT_SAME_INFO(rt_radiance_info, _reserved); RT_SAME_INFO(rt_visibility_info, mode);
#undef RT_SAME_FIELD
#undef RT_SAME_PARAMS
#undef RT_SAME_INFO

// One launch: `n` items from `in`, results to `out`, item 0 with stream index first_index
struct QuerySlice { const rtk::DeviceScene* S; const float4* in; void* out; int n; uint32_t first_index; int grid; LaneStack st; };

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
    bool sampled() const { return family < kClosest; }      // takes params and draws samples
    bool timed() const { return family != kRays; }          // has an info record with calls and kernel times
};

// A kernel's instantiation for the node form the renderer's kernels traverse (plan_launch): k<..., true> for compact nodes
template <class K> const void* pick_nodes(const rt_ctx* c, K* compact, K* plain)
{
    return c->opt_compact_nodes != 0 ? (const void*)compact : (const void*)plain;
}

// What the kernels that answer with a record start from (rtk::QueryHead's fields; QueryArgs has them under the same names)
template <class Args> void fill_head(const rt_ctx* c, const QuerySlice& s, Args& A)
{
    A.in = s.in;
    A.order = c->d_order.p;
    A.tri_mesh = c->geom_local ? c->d_tri_mesh.p : nullptr;
    A.intersect_mode = c->params.intersectMode;         // (zero-initialised params: RT_INTERSECT_FLAT_CHUNKS; k_closest does not read it)
}

// What the sampled kernels start from (rtk::SampledHead's fields, and the two every Args of theirs goes on with)
template <class Args> void fill_sampled(const rt_ctx* c, const QueryCall& q, const QuerySlice& s, Args& A)
{
    A.in = s.in; A.out = static_cast<float4*>(s.out);
    A.samples = q.p.samples; A.seed = q.p.seed; A.first_index = s.first_index; A.sample_lanes_log2 = q.sample_lanes_log2;
    A.full_sort = c->opt_full_sort;
}

// What every launch function ends with: the fields all the Args share, then the launch on the context's stream
template <class Args> hipError_t launch_slice(rt_ctx* c, const void* fn, const QuerySlice& s, Args& A)
{
    A.n = s.n; A.stack_cap = s.st.cap; A.gstack = s.st.gstack; A.gstack_stride = s.st.stride;
    void* args[] = { const_cast<rtk::DeviceScene*>(s.S), &A };
    return hipLaunchKernel(fn, dim3(s.grid), dim3(rtk::kBlock), args, s.st.lds, c->stream);
}

// n items in device memory -> n results, on the context's stream; no synchronisation.  One launch per q.slice items, each with the
// stream index advanced by the items before it (uint32_t: it wraps).
int launch_slices(rt_ctx* c, const QueryCall& q, const float4* in, void* out, int n, uint32_t first_index)
{
    rtk::DeviceScene S{};
    { int r = fill_scene(c, S); if (r) return r; }
    if (q.sampled()) {
        rt_gather_info& info = c->query_info[q.family];
        info.samples = q.p.samples; info.lastSampleLanes = 1 << q.sample_lanes_log2; info.mode = q.p.mode;
    }
    for (int first = 0; first < n; first += q.slice) {
        QuerySlice s{};
        s.S = &S; s.n = std::min(q.slice, n - first);
        const size_t lanes = (size_t)s.n << q.sample_lanes_log2;        // (a slice is at most 2^22 items: items * S stays below 2^31)
        s.grid = (int)((lanes + rtk::kBlock - 1) / rtk::kBlock);
        { int r = plan_lane_stack(c, (size_t)s.grid * rtk::kBlock, s.st, q.refuse_4g_for); if (r) return r; }
        s.in = in + 2 * (size_t)first; s.out = static_cast<char*>(out) + q.out_bytes * (size_t)first;
        s.first_index = first_index + (uint32_t)first;
        RT_HIP(c, q.launch(c, q, s));
    }
    return 0;
}

// Host memory in, host memory out: a slice at a time through the context's staging, sized to min(n, slice) items (an SH9 gather slice
// is 144 B per point).  The timed families time each slice's launches with the context's one event pair, so they wait for every
// slice before the next records the events again; ray queries record nothing and wait once, at the end.
int query_host(rt_ctx* c, const QueryCall& q, const rt_ray* in, int n, void* out)
{
    if (n == 0) return 0;
    { int r = query_prepare(c, query_origin_bound(in, n)); if (r) return r; }
    if (q.begin) { int r = q.begin(c); if (r) return r; }
    const size_t staged = (size_t)std::min(n, q.slice);
    RT_HIP(c, c->d_q_rays.ensure(2 * staged));
    RT_HIP(c, c->d_q_out.ensure(q.out_bytes * staged));
    double ms_sum = 0;
    for (int first = 0; first < n; first += q.slice) {
        const int cnt = std::min(q.slice, n - first);
        RT_HIP(c, hipMemcpyAsync(c->d_q_rays.p, in + first, (size_t)cnt * sizeof(rt_ray), hipMemcpyHostToDevice, c->stream));
        if (q.timed()) RT_HIP(c, hipEventRecord(c->ev0, c->stream));
        { int r = launch_slices(c, q, c->d_q_rays.p, c->d_q_out.p, cnt, q.p.firstIndex + (uint32_t)first); if (r) return r; }
        if (q.timed()) RT_HIP(c, hipEventRecord(c->ev1, c->stream));
        RT_HIP(c, hipMemcpyAsync(static_cast<char*>(out) + q.out_bytes * (size_t)first, c->d_q_out.p, q.out_bytes * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        if (!q.timed()) continue;
        RT_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        RT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_sum += ms;
    }
    if (!q.timed()) { RT_HIP(c, hipStreamSynchronize(c->stream)); return 0; }
    rt_gather_info& info = c->query_info[q.family];
    info.calls++; info.lastKernelMs = ms_sum; info.totalKernelMs += ms_sum;
    return 0;
}

// Device memory of the context's GPU in and out, ordered on the context's stream; the info record counts the call and keeps the host
// entry's times (the call is asynchronous)
int query_device(rt_ctx* c, const QueryCall& q, const void* in, int n, void* out)
{
    if (n == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    if (!on_ctx_device(c, in) || !on_ctx_device(c, out))
        return fail(c, -2, "%s: %s and results must be device memory of the context's device %d", q.what, q.in_word, c->device);
    if ((reinterpret_cast<uintptr_t>(in) & 15u) || (q.out_aligned && (reinterpret_cast<uintptr_t>(out) & 15u)))
        return fail(c, -2, "%s: %s%s%s must be 16-byte aligned", q.what, q.in_word, q.out_aligned ? " and " : "", q.out_aligned ? q.out_word : "");
    { int r = prepare_scene(c); if (r) return r; }
    { int r = cover_origins_device(c, static_cast<const float4*>(in), n); if (r) return r; }
    if (q.begin) { int r = q.begin(c); if (r) return r; }
    { int r = launch_slices(c, q, static_cast<const float4*>(in), out, n, q.p.firstIndex); if (r) return r; }
    if (q.timed()) c->query_info[q.family].calls++;
    return 0;
}

// ---- the six descriptions --------------------------------------------------------------------------------------------------------
// A *_call checks the arguments of a call to `what` and describes it; all have the signature of QueryDescribe (ray queries and
// closest-point queries take no params; multi-hit queries take their own, which are not the sampled families').  The checks come in one order: params set (where the family needs them), n and the pointers, the defaults of
// params == NULL, samples, mode, reserved words.
using QueryDescribe = int (*)(rt_ctx* c, const char* what, const void* in, int n, const void* params, const void* out, QueryCall& q);

int query_pointers(rt_ctx* c, const QueryCall& q, const void* in, int n, const void* out)
{
    if (n < 0 || (n > 0 && (!in || !out))) return fail(c, -2, "%s: bad arguments (n = %d, %s %p, %s %p)", q.what, n, q.in_word, in, q.out_word, out);
    return 0;
}

// The sampled families' common part.  modes: how many values of `mode` the family has, named by mode_text (radiance queries: one, and
// the word is a reserved one); params == NULL: default_samples samples, seed 0, firstIndex 0, mode 0.
int sampled_arguments(rt_ctx* c, QueryCall& q, bool need_params, const void* in, int n, const void* params, int default_samples, const void* out,
                      int modes, const char* mode_text, const char* params_type)
{
    if (need_params && !c->have_params) return fail(c, -2, "%s: rt_set_params has not been called", q.what);
    { int r = query_pointers(c, q, in, n, out); if (r) return r; }
    q.p = rt_gather_params{};
    if (params) std::memcpy(&q.p, params, sizeof q.p); else q.p.samples = default_samples;
    if (q.p.samples < 1 || q.p.samples > 65536) return fail(c, -2, "%s: samples = %d outside 1..65536", q.what, q.p.samples);
    q.sample_lanes_log2 = q.p.samples >= 16 ? 4 : q.p.samples >= 4 ? 2 : 0;
    if (mode_text && (q.p.mode < 0 || q.p.mode >= modes)) return fail(c, -2, "%s: mode = %d is %s", q.what, q.p.mode, mode_text);
    bool reserved = !mode_text && q.p.mode != 0;
    for (int r : q.p._reserved) reserved = reserved || r != 0;
    if (reserved) return fail(c, -2, "%s: a reserved word of %s is not 0", q.what, params_type);
    return 0;
}

template <bool ANY> hipError_t launch_rays(rt_ctx* c, const QueryCall&, const QuerySlice& s)
{
    if (c->opt_sweep) {                                     // sphere casts: the same rays, results and launch shape (csrc/rt_sweep.hpp)
        rtk::SweepArgs A{};
        fill_head(c, s, A);
        A.hits = ANY ? nullptr : static_cast<float4*>(s.out);
        A.occluded = ANY ? static_cast<uint8_t*>(s.out) : nullptr;
        return launch_slice(c, pick_nodes(c, rtk::k_sweep<ANY, true>, rtk::k_sweep<ANY, false>), s, A);
    }
    rtk::QueryArgs Q{};
    fill_head(c, s, Q);
    Q.full_sort = c->opt_full_sort;
    Q.hits = ANY ? nullptr : static_cast<float4*>(s.out);
    Q.occluded = ANY ? static_cast<uint8_t*>(s.out) : nullptr;
    return launch_slice(c, pick_nodes(c, rtk::k_ray_query<ANY, true>, rtk::k_ray_query<ANY, false>), s, Q);
}
// n rt_hit (4 float4 each) / n occlusion bytes
int trace_rays_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* hits, QueryCall& q)
{
    q = QueryCall{ kRays, what, "rays", "hits", kQuerySlice, sizeof(rt_hit), true, nullptr, launch_rays<false> };
    return query_pointers(c, q, rays, n, hits);
}
int occluded_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* occluded, QueryCall& q)
{
    q = QueryCall{ kRays, what, "rays", "occluded", kQuerySlice, 1, false, nullptr, launch_rays<true> };
    return query_pointers(c, q, rays, n, occluded);
}

hipError_t launch_radiance(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::RadianceArgs A{};
    fill_sampled(c, q, s, A);
    A.p = c->params;
    return launch_slice(c, pick_nodes(c, rtk::k_radiance<true>, rtk::k_radiance<false>), s, A);
}
// n float4; params == NULL: the context's numRaysPerPixel samples
int radiance_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* rgba, QueryCall& q)
{
    q = QueryCall{ kRadiance, what, "rays", "rgba", c->opt_radiance_slice, sizeof(float4), true, "rt_trace_radiance", launch_radiance };
    return sampled_arguments(c, q, true, rays, n, params, c->params.numRaysPerPixel, rgba, 1, nullptr, "rt_radiance_params");
}

hipError_t launch_gather(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::GatherArgs A{};
    fill_sampled(c, q, s, A);
    A.p = c->params;
    return launch_slice(c, q.p.mode == RT_GATHER_SH9 ? pick_nodes(c, rtk::k_gather<RT_GATHER_SH9, true>, rtk::k_gather<RT_GATHER_SH9, false>)
                                                     : pick_nodes(c, rtk::k_gather<RT_GATHER_COSINE, true>, rtk::k_gather<RT_GATHER_COSINE, false>), s, A);
}
// n or 9 n float4; params == NULL: the context's numRaysPerPixel samples
int gather_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q)
{
    q = QueryCall{ kGather, what, "points", "out", c->opt_gather_slice, 0, true, "rt_gather", launch_gather };
    { int r = sampled_arguments(c, q, true, points, n, params, c->params.numRaysPerPixel, out, 2, "neither RT_GATHER_COSINE nor RT_GATHER_SH9", "rt_gather_params"); if (r) return r; }
    q.out_bytes = sizeof(float4) * (q.p.mode == RT_GATHER_SH9 ? 9 : 1);
    return 0;
}

hipError_t launch_visibility(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::VisibilityArgs A{};
    fill_sampled(c, q, s, A);
    A.intersect_mode = c->params.intersectMode;         // (zero-initialised params: RT_INTERSECT_FLAT_CHUNKS)
    switch (q.p.mode) {
    case RT_VIS_SH9:      return launch_slice(c, pick_nodes(c, rtk::k_visibility<RT_VIS_SH9, true>, rtk::k_visibility<RT_VIS_SH9, false>), s, A);
    case RT_VIS_DISTANCE: return launch_slice(c, pick_nodes(c, rtk::k_visibility<RT_VIS_DISTANCE, true>, rtk::k_visibility<RT_VIS_DISTANCE, false>), s, A);
    default:              return launch_slice(c, pick_nodes(c, rtk::k_visibility<RT_VIS_COSINE, true>, rtk::k_visibility<RT_VIS_COSINE, false>), s, A);
    }
}
// n or 3 n float4; params == NULL: RT_VISIBILITY_DEFAULT_SAMPLES samples.  No rt_params are needed: the kernel reads intersectMode
// alone, as the ray queries do
int visibility_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q)
{
    q = QueryCall{ kVisibility, what, "points", "out", c->opt_visibility_slice, 0, true, "rt_visibility", launch_visibility };
    { int r = sampled_arguments(c, q, false, points, n, params, RT_VISIBILITY_DEFAULT_SAMPLES, out, 3, "none of RT_VIS_COSINE, RT_VIS_SH9, RT_VIS_DISTANCE", "rt_visibility_params"); if (r) return r; }
    q.out_bytes = sizeof(float4) * (q.p.mode == RT_VIS_SH9 ? 3 : 1);
    return 0;
}

// Counting calls start from zero; the sums stay on the device until rt_get_closest_info asks for them (the device entry does not wait)
int begin_closest(rt_ctx* c)
{
    c->closest_counts[0] = c->closest_counts[1] = 0;
    c->closest_counts_pending = false;
    if (!c->opt_closest_count) return 0;
    RT_HIP(c, c->d_closest_counts.ensure(2));
    RT_HIP(c, hipMemsetAsync(c->d_closest_counts.p, 0, 2 * sizeof(unsigned long long), c->stream));
    c->closest_counts_pending = true;
    return 0;
}
// k_closest, k_nearest or k_overlap<node form, counting>
template <bool COUNT> const void* pick_closest(const rt_ctx* c, bool nearest, bool box)
{
    return box     ? pick_nodes(c, rtk::k_overlap<true, COUNT>, rtk::k_overlap<false, COUNT>)
         : nearest ? pick_nodes(c, rtk::k_nearest<true, COUNT>, rtk::k_nearest<false, COUNT>)
                   : pick_nodes(c, rtk::k_closest<true, COUNT>, rtk::k_closest<false, COUNT>);
}
hipError_t launch_closest(rt_ctx* c, const QueryCall&, const QuerySlice& s)
{
    // K-nearest queries: the same points and launch shape, K records each (csrc/rt_nearest.hpp); k_closest takes the Args' ClosestArgs part
    // box overlap queries ("closest_box" = 1): each input is a box, whatever K and all are (csrc/rt_overlap.hpp)
    const bool nearest = c->opt_closest_k != 1 || c->opt_closest_all, box = c->opt_closest_box != 0;
    rtk::NearestArgs A{};
    fill_head(c, s, A);
    A.out = static_cast<float4*>(s.out);
    A.counters = c->opt_closest_count ? c->d_closest_counts.p : nullptr;
    A.k = c->opt_closest_k; A.count_all = c->opt_closest_all;
    return launch_slice(c, c->opt_closest_count ? pick_closest<true>(c, nearest, box) : pick_closest<false>(c, nearest, box), s, A);
}
// n * K rt_closest (4 float4 each), K = option "closest_k"; no params of either kind.  The points per launch are min("closest_slice",
// 4194304 / K): the staged results never exceed the 256 MiB of K = 1
int closest_call(rt_ctx* c, const char* what, const void* points, int n, const void*, const void* out, QueryCall& q)
{
    const int K = c->opt_closest_k;
    q = QueryCall{ kClosest, what, "points", "out", std::min(c->opt_closest_slice, kQuerySlice / K), sizeof(rt_closest) * (size_t)K, true, nullptr, launch_closest };
    q.begin = begin_closest;
    return query_pointers(c, q, points, n, out);
}

hipError_t launch_hits(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::MultihitArgs A{};
    fill_head(c, s, A);
    A.max_hits = q.h.maxHits; A.count_all = q.h.countAll;
    A.out = static_cast<float4*>(s.out);
    c->hits_last = q.h;
    if (q.h.mode == RT_HITS_BOTH) return launch_slice(c, pick_nodes(c, rtk::k_multihit<true, true>, rtk::k_multihit<false, true>), s, A);
    return launch_slice(c, pick_nodes(c, rtk::k_multihit<true, false>, rtk::k_multihit<false, false>), s, A);
}
// n * K rt_multihit (4 float4 each); params == NULL: RT_HITS_DEFAULT_MAX records per ray, front faces, hitCount capped at K.  No
// rt_params are needed: the kernel reads intersectMode alone, as the ray queries do
int hits_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* out, QueryCall& q)
{
    q = QueryCall{ kHits, what, "rays", "out", c->opt_hits_slice, 0, true, nullptr, launch_hits };
    { int r = query_pointers(c, q, rays, n, out); if (r) return r; }
    if (params) std::memcpy(&q.h, params, sizeof q.h); else q.h.maxHits = RT_HITS_DEFAULT_MAX;
    if (q.h.maxHits < 1 || q.h.maxHits > RT_HITS_MAX) return fail(c, -2, "%s: maxHits = %d outside 1..%d", what, q.h.maxHits, RT_HITS_MAX);
    if (q.h.mode != RT_HITS_FRONT && q.h.mode != RT_HITS_BOTH) return fail(c, -2, "%s: mode = %d is neither RT_HITS_FRONT nor RT_HITS_BOTH", what, q.h.mode);
    if (q.h.countAll != 0 && q.h.countAll != 1) return fail(c, -2, "%s: countAll = %d is neither 0 nor 1", what, q.h.countAll);
    for (int r : q.h._reserved) if (r != 0) return fail(c, -2, "%s: a reserved word of rt_hits_params is not 0", what);
    q.out_bytes = sizeof(rt_multihit) * (size_t)q.h.maxHits;
    return 0;
}

// Every exported query entry of a context: settle, check and describe, then the host or the device path
int query_entry(rt_ctx* c, QueryDescribe describe, const char* what, bool device, const void* in, int n, const void* params, void* out)
{
    if (!c) return -1;
    RT_SETTLE(c);
    QueryCall q;
    { int r = describe(c, what, in, n, params, out, q); if (r) return r; }
    return device ? query_device(c, q, in, n, out) : query_host(c, q, static_cast<const rt_ray*>(in), n, out);
}

// ---- feature buffers (rt_render_aov, csrc/rt_aov.hpp) -----------------------------------------------------------------------------
// The two planes of the context's strip, zeroed when they are created and whenever the strip's layout changes (ensure_targets' rule for
// the accumulation target, kept apart from it: a feature frame must not touch the image path's state)
bool aov_current(const rt_ctx* c, const StripLayout& L) { return c->d_aov[0].p && L == c->aov; }
int ensure_aov(rt_ctx* c)
{
    StripLayout L;
    { int r = strip_layout(c, L); if (r) return r; }
    if (aov_current(c, L)) return 0;
    static_assert(RT_AOV_COUNT == 2, "the planes listed below");
    { int r = create_planes(c, L, { &c->d_aov[0], &c->d_aov[1] }); if (r) return r; }
    c->aov = L;
    c->aov_info.framesAccumulated = 0; c->aov_info.totalKernelMs = 0;
    return 0;
}

int render_aov(rt_ctx* c, int first_frame, int n_frames)
{
    RT_SETTLE(c);
    if (!c->have_params) return fail(c, -2, "rt_render_aov: rt_set_params has not been called");
    if (n_frames < 0) return fail(c, -2, "rt_render_aov: n_frames < 0");
    if (n_frames == 0) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    { int r = prepare_scene(c); if (r) return r; }
    { int r = ensure_aov(c); if (r) return r; }
    rtk::DeviceScene S{};
    { int r = fill_scene(c, S); if (r) return r; }
    rtk::AovArgs A{};
    A.p = c->params;
    A.row0 = c->aov.row0; A.nrows = c->aov.rows; A.row_stride = c->aov.row_stride;
    // S = 16 / 4 / 1 sub-streams of a pixel on adjacent lanes: a wave is a 2x2 / 4x4 / 8x8 tile (all divide the 8-row bands)
    const int N = c->params.numRaysPerPixel;
    A.sample_lanes_log2 = N >= 16 ? 4 : N >= 4 ? 2 : 0;
    const int tile = 1 << ((6 - A.sample_lanes_log2) / 2);
    const long long tiles_x = (c->aov.w + tile - 1) / tile, tiles_y = (c->aov.rows + tile - 1) / tile;
    c->aov_info.lastSampleLanes = 1 << A.sample_lanes_log2;
    if (tiles_x * tiles_y == 0) { c->aov_info.framesAccumulated += n_frames; c->aov_info.lastKernelMs = 0; return 0; }
    if (tiles_x * tiles_y > (long long)1 << 30) return fail(c, -7, "rt_render_aov: %lld wave tiles exceed one launch", tiles_x * tiles_y);
    A.tiles_x = (int)tiles_x; A.ntiles = (int)(tiles_x * tiles_y);
    A.full_sort = c->opt_full_sort;
    A.fixed_origin = camera_origin_is_fixed(c->params) ? 1 : 0;
    A.albedo = c->d_aov[RT_AOV_ALBEDO].p; A.normal_depth = c->d_aov[RT_AOV_NORMAL_DEPTH].p;
    const int grid = (A.ntiles + rtk::kWavesPerBlock - 1) / rtk::kWavesPerBlock;
    LaneStack st;
    { int r = plan_lane_stack(c, (size_t)grid * rtk::kBlock, st, "rt_render_aov"); if (r) return r; }
    A.stack_cap = st.cap; A.gstack = st.gstack; A.gstack_stride = st.stride;
    const void* fn = pick_nodes(c, rtk::k_aov<true>, rtk::k_aov<false>);
    RT_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int f = 0; f < n_frames; ++f) {
        A.frame = first_frame + f; A.accumulated = c->aov_info.framesAccumulated + f;
        void* args[] = { &S, &A };
        RT_HIP(c, hipLaunchKernel(fn, dim3(grid), dim3(rtk::kBlock), args, st.lds, c->stream));
    }
    RT_HIP(c, hipEventRecord(c->ev1, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    RT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->aov_info.framesAccumulated += n_frames; c->aov_info.lastKernelMs = ms; c->aov_info.totalKernelMs += ms;
    return 0;
}

int read_aov(rt_ctx* c, int which, void* dst, size_t n_floats, bool to_device)
{
    RT_SETTLE(c);
    if (which < 0 || which >= RT_AOV_COUNT) return fail(c, -2, "unknown feature plane %d", which);
    if (!c->have_params) return fail(c, -2, "rt_set_params has not been called");
    if (!dst) return fail(c, -2, "null destination");
    RT_HIP(c, hipSetDevice(c->device));
    { int r = ensure_aov(c); if (r) return r; }
    return copy_plane(c, c, c->d_aov[which].p, c->aov.pixels() * 4, "rows*width*4", dst, n_floats, to_device);
}

// ---- the image filters' one host path -----------------------------------------------------------------------------------
// rt_denoise, rt_temporal, rt_denoise_temporal, rt_denoise_variance and their rt_multi_ forms are each: begin_filter, the filter's
// validator, filter_inputs, the filter's run_*.  A context and a handle differ in the two overloads of begin_filter and filter_inputs (and
// in the order of their checks); everything else below is written once.

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

// The temporal colour as a filter's source: T exists and has the image's size.  `temporal` is the call that makes T and `whose` the
// owner of the image in the messages ("context's" / "handle's")
int temporal_source(ErrOwner* o, const TemporalPlanes& T, int W, int H, const FilterCall& k, const char* temporal, const char* whose)
{
    if (!T.filled) return fail(o, -2, "%s: %s%s has not been called", k.what, k.lead, temporal);
    if (T.w != W || T.h != H) return fail(o, -2, "%s: the temporal image is %d x %d, the %s image %d x %d", k.what, T.w, T.h, whose, W, H);
    return 0;
}

// A context may run the call: settled, with params ...
int begin_filter(rt_ctx* c, const char* what)
{
    RT_SETTLE(c);
    return c->have_params ? 0 : fail(c, -2, "%s: rt_set_params has not been called", what);
}
// ... and it holds the whole image and current feature planes with a frame in them (planes of another layout would be re-created,
// zeroed); then T, if that is the source (from_T) and not the image; then the inputs on its device (the image is a cleared one if it was
// never created at this size)
int filter_inputs(rt_ctx* c, const FilterCall& k, bool from_T, FilterInputs& I)
{
    StripLayout L;
    { int r = strip_layout(c, L); if (r) return r; }
    if (c->band_stride > 1 || L.row0 != 0 || L.rows != L.h)
        return fail(c, -2, "%s: the context holds rows of the image, not the whole image (%d of %d rows); use %s", k.what, L.rows, L.h, k.use_instead);
    if (!aov_current(c, L) || c->aov_info.framesAccumulated == 0) return fail(c, -2, "%s: no feature frame accumulated (call rt_render_aov first)", k.what);
    if (from_T) { int r = temporal_source(c, c->tp, L.w, L.h, k, "rt_temporal", "context's"); if (r) return r; }
    RT_HIP(c, hipSetDevice(c->device));
    if (!from_T) { int r = ensure_targets(c); if (r) return r; }
    I.C = from_T ? c->tp.t[c->tp.cur].p : c->d_accum.p; I.A = c->d_aov[RT_AOV_ALBEDO].p; I.G = c->d_aov[RT_AOV_NORMAL_DEPTH].p;
    I.W = L.w; I.H = L.h; I.cam = &c->params;
    I.stream = c->stream; I.ev0 = c->ev_dn0; I.ev1 = c->ev_dn1;
    return 0;
}
// (the handle's two are defined with the handle, below)
int begin_filter(rt_multi* m, const char* what);
int filter_inputs(rt_multi* m, const FilterCall& k, bool from_T, FilterInputs& I);

// `launches` on `stream` between ev0 and ev1, waited for -> their time
template <class Fn> hipError_t timed(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, float& ms, Fn launches)
{
    hipError_t e;
    if ((e = hipEventRecord(ev0, stream)) != hipSuccess) return e;
    launches();
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(ev1, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    return hipEventElapsedTime(&ms, ev0, ev1);
}

// The pieces the validators are made of.  A validator gives P the caller's parameters or the defaults, and returns nullptr, or why they
// are out of range
bool is_flag(int v) { return v == 0 || v == 1; }
bool finite_and_positive(std::initializer_list<float> values)
{
    for (float v : values) if (!std::isfinite(v) || !(v > 0.0f)) return false;
    return true;
}
const char* atrous_params(int iterations, int demodulate)           // what both A-trous filters take
{
    if (iterations < 1 || iterations > 6) return "iterations outside 1..6";
    return is_flag(demodulate) ? nullptr : "demodulate is neither 0 nor 1";
}

// The readers of a filter's plane S (`call`: the call that fills it), for the owner o whose plane it is, on the context `on` that holds
// it (copy_plane).  `per` floats per pixel: 4 or 1
int readable(ErrOwner* o, const FilterPlanes& S, const char* call, const void* dst)
{
    if (!S.filled) return fail(o, -2, "%s has not been called", call);
    return dst ? 0 : fail(o, -2, "null destination");
}
int read_filter_plane(ErrOwner* o, const rt_ctx* on, const FilterPlanes& S, const char* call, const void* src, int per, void* dst, size_t n_floats, bool to_device)
{
    { int r = readable(o, S, call, dst); if (r) return r; }
    return copy_plane(o, on, src, S.pixels() * per, per == 4 ? "height*width*4" : "height*width", dst, n_floats, to_device);
}

// The display step: linear -> sRGB8 of a plane of n_pixels > 0 on c's device (already current), through `display` there, on c's stream;
// kernel_ms, if asked for, is the kernel's time
hipError_t display_plane(rt_ctx* c, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels, float* kernel_ms = nullptr)
{
    hipError_t e = display.ensure(n_pixels);
    if (e != hipSuccess) return e;
    if (kernel_ms && (e = hipEventRecord(c->evg0, c->stream)) != hipSuccess) return e;
    const int grid = (int)std::min<size_t>((n_pixels + 255) / 256, (size_t)std::max(1, c->n_cu) * 8);
    hipLaunchKernelGGL(rtg::k_display_srgb8, dim3(grid), dim3(256), 0, c->stream, plane, display.p, n_pixels);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (kernel_ms && (e = hipEventRecord(c->evg1, c->stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(rgba8, display.p, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    return kernel_ms ? hipEventElapsedTime(kernel_ms, c->evg0, c->evg1) : hipSuccess;
}

// The end of every read of a whole-image plane as sRGB8: n_pixels must be its `pixels`, then the display step on `on` (as copy_plane).
// A plane that is still null is the handle's image before the first render
int read_srgb8(ErrOwner* o, rt_ctx* on, const float4* plane, size_t pixels, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels)
{
    if (n_pixels != pixels) return fail(o, -2, "expected %zu pixels (height*width), got %zu", pixels, n_pixels);
    if (!n_pixels) return 0;
    if (!plane) return fail(o, -2, "nothing rendered yet");
    RT_HIP(o, hipSetDevice(on->device));
    RT_HIP(o, display_plane(on, plane, display, rgba8, n_pixels));
    return 0;
}
int read_filter_display(ErrOwner* o, rt_ctx* on, const FilterPlanes& S, const char* call, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels)
{
    { int r = readable(o, S, call, rgba8); if (r) return r; }
    return read_srgb8(o, on, plane, S.pixels(), display, rgba8, n_pixels);
}

// a context's reads of its own filter planes (the queue settled first)
enum class OwnPlane { Denoised, Temporal, History, Variance };
int read_own(rt_ctx* c, OwnPlane which, void* dst, size_t n_floats, bool to_device)
{
    if (!c) return -1;
    RT_SETTLE(c);
    switch (which) {
    case OwnPlane::Denoised: return read_filter_plane(c, c, c->dn, "rt_denoise", c->dn.out.p, 4, dst, n_floats, to_device);
    case OwnPlane::Temporal: return read_filter_plane(c, c, c->tp, "rt_temporal", c->tp.t[c->tp.cur].p, 4, dst, n_floats, to_device);
    case OwnPlane::History:  return read_filter_plane(c, c, c->tp, "rt_temporal", c->tp.n[c->tp.cur].p, 1, dst, n_floats, to_device);
    default:                 return read_filter_plane(c, c, c->vd, "rt_denoise_variance", c->vd.var.p, 1, dst, n_floats, to_device);
    }
}

// a context's info record (the queue settled first)
template <class Info> int read_info(rt_ctx* c, const Info& info, Info* out)
{
    RT_SETTLE(c);
    if (!out) return fail(c, -2, "null info");
    *out = info;
    return 0;
}

// ---- denoiser (rt_denoise, csrc/rt_denoise.hpp) -----------------------------------------------------------------------------------
static_assert(sizeof(rt_denoise_params) == 32 && sizeof(rt_denoise_info) == 32, "denoiser ABI");

const char* denoise_params(const rt_denoise_params* in, rt_denoise_params& P)
{
    P = rt_denoise_params{};
    P.iterations = RT_DENOISE_DEFAULT_ITERATIONS; P.demodulate = RT_DENOISE_DEFAULT_DEMODULATE;
    P.sigmaColour = RT_DENOISE_DEFAULT_SIGMA_COLOUR; P.sigmaNormal = RT_DENOISE_DEFAULT_SIGMA_NORMAL; P.sigmaDepth = RT_DENOISE_DEFAULT_SIGMA_DEPTH;
    if (in) P = *in;
    if (const char* why = atrous_params(P.iterations, P.demodulate)) return why;
    return finite_and_positive({ P.sigmaColour, P.sigmaNormal, P.sigmaDepth }) ? nullptr : "a sigma is not finite or not > 0";
}

// What both A-trous filters start with (inside their timed launches): e_0 and d from C and A, then the passes' tile grid and the
// guide weights' factors
struct AtrousStart { dim3 grid; float kn, kz; };
AtrousStart atrous_start(DenoisePlanes& D, const FilterInputs& I, int demodulate, float sigmaNormal, float sigmaDepth)
{
    const size_t px = I.pixels();
    hipLaunchKernelGGL(rtk::k_denoise_prep, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, I.stream, I.C, I.A, D.e[0].p, D.d.p, px, demodulate);
    return { dim3((I.W + rtk::kDenoiseTileW - 1) / rtk::kDenoiseTileW, (I.H + rtk::kDenoiseTileH - 1) / rtk::kDenoiseTileH),
             1.0f / (sigmaNormal * sigmaNormal), 1.0f / (sigmaDepth * sigmaDepth) };
}

// The filter: I -> D.out; P has passed denoise_params
hipError_t run_denoise(DenoisePlanes& D, const FilterInputs& I, const rt_denoise_params& P)
{
    hipError_t e = D.at(I.W, I.H);
    if (e != hipSuccess) return e;
    float ms = 0.f;
    if (I.pixels()) e = timed(I.stream, I.ev0, I.ev1, ms, [&] {
        const AtrousStart s = atrous_start(D, I, P.demodulate, P.sigmaNormal, P.sigmaDepth);
        const float kc0 = 1.0f / (P.sigmaColour * P.sigmaColour);
        for (int i = 0; i < P.iterations; ++i) {
            const bool last = i == P.iterations - 1;
            rtk::AtrousArgs a{};
            a.e_in = D.e[i & 1].p; a.guide = I.G; a.d = D.d.p; a.e_out = last ? D.out.p : D.e[(i + 1) & 1].p;
            a.W = I.W; a.H = I.H; a.step = 1 << i;
            a.kn = s.kn; a.kz = s.kz; a.kc = kc0 * (float)(1 << (2 * i));
            if (last) hipLaunchKernelGGL(rtk::k_atrous<true>, s.grid, dim3(256), 0, I.stream, a);
            else hipLaunchKernelGGL(rtk::k_atrous<false>, s.grid, dim3(256), 0, I.stream, a);
        }
    });
    if (e != hipSuccess) return e;
    D.filled = true;
    D.info.iterations = P.iterations; D.info.demodulate = P.demodulate; D.info.width = I.W; D.info.height = I.H;
    D.info.lastKernelMs = ms; D.info.totalKernelMs += ms;
    return hipSuccess;
}

// rt_denoise, rt_denoise_temporal (from_T) and their rt_multi_ forms
template <class Owner> int denoise_call(Owner* o, const FilterCall& k, bool from_T, const rt_denoise_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_denoise_params P;
    if (const char* why = denoise_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, from_T, I); if (r) return r; }
    RT_HIP(o, run_denoise(o->dn, I, P));
    return 0;
}

// ---- temporal reprojection (rt_temporal, csrc/rt_temporal.hpp) --------------------------------------------------------------------
static_assert(sizeof(rt_temporal_params) == 32 && sizeof(rt_temporal_info) == 32, "temporal ABI");

const char* temporal_params(const rt_temporal_params* in, rt_temporal_params& P)
{
    P = rt_temporal_params{};
    P.maxHistory = RT_TEMPORAL_DEFAULT_MAX_HISTORY;
    P.depthTolerance = RT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE; P.normalTolerance = RT_TEMPORAL_DEFAULT_NORMAL_TOLERANCE;
    if (in) P = *in;
    if (P.maxHistory < 1 || P.maxHistory > 4096) return "maxHistory outside 1..4096";
    return finite_and_positive({ P.depthTolerance, P.normalTolerance }) ? nullptr : "a tolerance is not finite or not > 0";
}

// The step: I (and its camera) -> the other pair of S's planes; P has passed temporal_params.  Without history (call 0) N' is zeroed, so
// no tap counts, and the previous camera is this call's.
hipError_t run_temporal(TemporalPlanes& S, const FilterInputs& I, const rt_temporal_params& P)
{
    const size_t px = I.pixels();
    const rt_params& cam = *I.cam;
    hipError_t e = S.at(I.W, I.H);
    if (e != hipSuccess) return e;
    const int prev = S.cur, next = S.cur ^ 1;
    float ms = 0.f;
    if (px) {
        if (!S.filled) {            // no history: T', N' and G' read as zero
            if ((e = hipMemsetAsync(S.t[prev].p, 0, px * sizeof(float4), I.stream)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(S.g[prev].p, 0, px * sizeof(float4), I.stream)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(S.n[prev].p, 0, px * sizeof(float), I.stream)) != hipSuccess) return e;
        }
        const rt_params& pc = S.filled ? S.cam : cam;
        rtk::TemporalArgs a{};
        a.C = I.C; a.A = I.A; a.G = I.G;
        a.Tp = S.t[prev].p; a.Np = S.n[prev].p; a.Gp = S.g[prev].p;
        a.T = S.t[next].p; a.N = S.n[next].p; a.Gn = S.g[next].p;
        a.W = I.W; a.H = I.H;
        for (int i = 0; i < 12; ++i) a.M[i] = cam.camLocalToWorld[i];
        const float* Mp = pc.camLocalToWorld;
        for (int i = 0; i < 3; ++i) {
            a.O[i] = cam.worldSpaceCameraPos[i]; a.V[i] = cam.viewParams[i];
            a.pO[i] = pc.worldSpaceCameraPos[i]; a.pV[i] = pc.viewParams[i];
            a.pt[i] = Mp[4 * i + 3];
            const float cx = Mp[i], cy = Mp[4 + i], cz = Mp[8 + i];
            a.pc[i][0] = cx; a.pc[i][1] = cy; a.pc[i][2] = cz;
            a.pcc[i] = (cx * cx + cy * cy) + cz * cz;
        }
        a.depthTol = P.depthTolerance; a.normalTol2 = P.normalTolerance * P.normalTolerance; a.maxHistory = (float)P.maxHistory;
        const dim3 grid((I.W + rtk::kTemporalTileW - 1) / rtk::kTemporalTileW, (I.H + rtk::kTemporalTileH - 1) / rtk::kTemporalTileH);
        if ((e = timed(I.stream, I.ev0, I.ev1, ms, [&] { hipLaunchKernelGGL(rtk::k_temporal, grid, dim3(256), 0, I.stream, a); })) != hipSuccess) return e;
    }
    S.cur = next; S.filled = true; S.cam = cam;
    S.info.calls += 1; S.info.width = I.W; S.info.height = I.H;
    S.info.lastKernelMs = ms; S.info.totalKernelMs += ms;
    return hipSuccess;
}

// rt_temporal and rt_multi_temporal
template <class Owner> int temporal_call(Owner* o, const FilterCall& k, const rt_temporal_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_temporal_params P;
    if (const char* why = temporal_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, false, I); if (r) return r; }
    RT_HIP(o, run_temporal(o->tp, I, P));
    return 0;
}

// ---- variance-guided denoiser (rt_denoise_variance, csrc/rt_vdenoise.hpp) -----------------------------------------------------------
static_assert(sizeof(rt_vdenoise_params) == 32 && sizeof(rt_vdenoise_info) == 32, "variance-guided denoiser ABI");

const char* vdenoise_params(const rt_vdenoise_params* in, rt_vdenoise_params& P)
{
    P = rt_vdenoise_params{};
    P.iterations = RT_VDENOISE_DEFAULT_ITERATIONS; P.demodulate = RT_VDENOISE_DEFAULT_DEMODULATE;
    P.sigmaLuminance = RT_VDENOISE_DEFAULT_SIGMA_LUMINANCE; P.sigmaNormal = RT_VDENOISE_DEFAULT_SIGMA_NORMAL; P.sigmaDepth = RT_VDENOISE_DEFAULT_SIGMA_DEPTH;
    if (in) P = *in;
    if (const char* why = atrous_params(P.iterations, P.demodulate)) return why;
    if (!is_flag(P.source)) return "source is neither 0 nor 1";
    if (!finite_and_positive({ P.sigmaLuminance, P.sigmaNormal, P.sigmaDepth })) return "a sigma is not finite or not > 0";
    return P._reserved[0] == 0 && P._reserved[1] == 0 ? nullptr : "a reserved word is not 0";
}

// The filter: I -> D.out and V.var, through D's work planes; P has passed vdenoise_params
hipError_t run_vdenoise(DenoisePlanes& D, VariancePlane& V, const FilterInputs& I, const rt_vdenoise_params& P)
{
    hipError_t e;
    if ((e = D.at(I.W, I.H)) != hipSuccess || (e = V.at(I.W, I.H)) != hipSuccess) return e;
    float ms = 0.f;
    if (I.pixels()) e = timed(I.stream, I.ev0, I.ev1, ms, [&] {
        const AtrousStart s = atrous_start(D, I, P.demodulate, P.sigmaNormal, P.sigmaDepth);
        rtk::VarEstimateArgs v{};
        v.e0 = D.e[0].p; v.guide = I.G; v.e_out = D.e[1].p; v.var = V.var.p; v.W = I.W; v.H = I.H; v.kn = s.kn; v.kz = s.kz;
        hipLaunchKernelGGL(rtk::k_variance_estimate, s.grid, dim3(256), 0, I.stream, v);
        for (int i = 0; i < P.iterations; ++i) {            // (e_0, var_0) is in e[1]: pass i reads e[(i + 1) & 1]
            const bool last = i == P.iterations - 1;
            rtk::VarAtrousArgs a{};
            a.e_in = D.e[(i + 1) & 1].p; a.guide = I.G; a.d = D.d.p; a.e_out = last ? D.out.p : D.e[i & 1].p;
            a.W = I.W; a.H = I.H; a.step = 1 << i;
            a.kn = s.kn; a.kz = s.kz; a.sl = P.sigmaLuminance;
            if (last) hipLaunchKernelGGL(rtk::k_var_atrous<true>, s.grid, dim3(256), 0, I.stream, a);
            else hipLaunchKernelGGL(rtk::k_var_atrous<false>, s.grid, dim3(256), 0, I.stream, a);
        }
    });
    if (e != hipSuccess) return e;
    D.filled = true; V.filled = true;
    V.info.iterations = P.iterations; V.info.source = P.source; V.info.width = I.W; V.info.height = I.H;
    V.info.lastKernelMs = ms; V.info.totalKernelMs += ms;
    return hipSuccess;
}

// rt_denoise_variance and rt_multi_denoise_variance (source 1: the temporal colour)
template <class Owner> int denoise_variance_call(Owner* o, const FilterCall& k, const rt_vdenoise_params* in)
{
    if (!o) return -1;
    { int r = begin_filter(o, k.what); if (r) return r; }
    rt_vdenoise_params P;
    if (const char* why = vdenoise_params(in, P)) return fail(o, -2, "%s: %s", k.what, why);
    FilterInputs I;
    { int r = filter_inputs(o, k, P.source == 1, I); if (r) return r; }
    RT_HIP(o, run_vdenoise(o->dn, o->vd, I, P));
    return 0;
}

} // namespace

extern "C" {

int rt_abi_version(void) { return 1; }

int rt_sizeof(const char* name)
{
    if (!name) return -1;
    if (!std::strcmp(name, "rt_material")) return (int)sizeof(rt_material);
    if (!std::strcmp(name, "rt_sphere"))   return (int)sizeof(rt_sphere);
    if (!std::strcmp(name, "rt_triangle")) return (int)sizeof(rt_triangle);
    if (!std::strcmp(name, "rt_meshinfo")) return (int)sizeof(rt_meshinfo);
    if (!std::strcmp(name, "rt_params"))   return (int)sizeof(rt_params);
    if (!std::strcmp(name, "rt_stats"))    return (int)sizeof(rt_stats);
    if (!std::strcmp(name, "rt_mesh_transform")) return (int)sizeof(rt_mesh_transform);
    if (!std::strcmp(name, "rt_local_chunk")) return (int)sizeof(rt_local_chunk);
    if (!std::strcmp(name, "rt_multi_info")) return (int)sizeof(rt_multi_info);
    if (!std::strcmp(name, "rt_ray")) return (int)sizeof(rt_ray);
    if (!std::strcmp(name, "rt_hit")) return (int)sizeof(rt_hit);
    if (!std::strcmp(name, "rt_aov_info")) return (int)sizeof(rt_aov_info);
    if (!std::strcmp(name, "rt_denoise_params")) return (int)sizeof(rt_denoise_params);
    if (!std::strcmp(name, "rt_denoise_info")) return (int)sizeof(rt_denoise_info);
    if (!std::strcmp(name, "rt_temporal_params")) return (int)sizeof(rt_temporal_params);
    if (!std::strcmp(name, "rt_temporal_info")) return (int)sizeof(rt_temporal_info);
    if (!std::strcmp(name, "rt_vdenoise_params")) return (int)sizeof(rt_vdenoise_params);
    if (!std::strcmp(name, "rt_vdenoise_info")) return (int)sizeof(rt_vdenoise_info);
    if (!std::strcmp(name, "rt_radiance_params")) return (int)sizeof(rt_radiance_params);
    if (!std::strcmp(name, "rt_radiance_info")) return (int)sizeof(rt_radiance_info);
    if (!std::strcmp(name, "rt_gather_params")) return (int)sizeof(rt_gather_params);
    if (!std::strcmp(name, "rt_gather_info")) return (int)sizeof(rt_gather_info);
    if (!std::strcmp(name, "rt_visibility_params")) return (int)sizeof(rt_visibility_params);
    if (!std::strcmp(name, "rt_visibility_info")) return (int)sizeof(rt_visibility_info);
    if (!std::strcmp(name, "rt_closest")) return (int)sizeof(rt_closest);
    if (!std::strcmp(name, "rt_closest_info")) return (int)sizeof(rt_closest_info);
    if (!std::strcmp(name, "rt_hits_params")) return (int)sizeof(rt_hits_params);
    if (!std::strcmp(name, "rt_multihit")) return (int)sizeof(rt_multihit);
    if (!std::strcmp(name, "rt_hits_info")) return (int)sizeof(rt_hits_info);
    return -1;
}

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

rt_ctx* rt_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { fail(nullptr, -1, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e)); return nullptr; }
    if (device < 0 || device >= n) { fail(nullptr, -1, "device %d out of range [0,%d)", device, n); return nullptr; }
    if ((e = hipSetDevice(device)) != hipSuccess) { fail(nullptr, -1, "hipSetDevice: %s", hipGetErrorString(e)); return nullptr; }
    rt_ctx* c = new rt_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) { fail(nullptr, -1, "hipGetDeviceProperties: %s", hipGetErrorString(e)); delete c; return nullptr; }
    c->n_cu = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess
        || (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess
        || (e = hipEventCreate(&c->evg0)) != hipSuccess || (e = hipEventCreate(&c->evg1)) != hipSuccess
        || (e = hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming)) != hipSuccess
        || (e = hipEventCreate(&c->ev_dn0)) != hipSuccess || (e = hipEventCreate(&c->ev_dn1)) != hipSuccess
        || (e = hipMalloc((void**)&c->d_tile_counter, sizeof(unsigned int))) != hipSuccess
        || (e = hipMalloc((void**)&c->d_counters, rtk::kNumCounters * sizeof(unsigned long long))) != hipSuccess) {
        fail(nullptr, -1, "context setup: %s", hipGetErrorString(e));
        rt_destroy(c);
        return nullptr;
    }
    c->stream = c->own_stream;
    return c;
}

void rt_destroy(rt_ctx* c)
{
    if (!c) return;
    if (c->q_started) {
        { std::lock_guard<std::mutex> lk(c->q_mu); c->q_stop = true; }
        c->q_cv.notify_all();
        c->q_thread.join();
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_tile_counter) (void)hipFree(c->d_tile_counter);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->evg0) (void)hipEventDestroy(c->evg0);
    if (c->evg1) (void)hipEventDestroy(c->evg1);
    if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
    if (c->ev_dn0) (void)hipEventDestroy(c->ev_dn0);
    if (c->ev_dn1) (void)hipEventDestroy(c->ev_dn1);
    c->bvh_ws.release();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                           // (every DevBuf frees itself, on the device made current above)
}

int rt_set_stream(rt_ctx* c, void* hip_stream)
{
    if (!c) return -1;
    RT_SETTLE(c);
    const hipStream_t next = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (next != c->stream) {
        // ordered switch: what the context enqueued on the outgoing stream (a device query, say) completes before anything it enqueues
        // on the incoming one — its buffers (scene, staging, traversal-stack overflow) are shared by the work of both
        RT_HIP(c, hipSetDevice(c->device));
        RT_HIP(c, hipEventRecord(c->ev_switch, c->stream));
        RT_HIP(c, hipStreamWaitEvent(next, c->ev_switch, 0));
        c->stream = next;
    }
    return 0;
}

int rt_set_params(rt_ctx* c, const rt_params* p)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!p) return fail(c, -2, "null params");
    if (p->width < 0 || p->height < 0 || (int64_t)p->width * p->height > (int64_t)1 << 31) return fail(c, -2, "bad target size %dx%d", p->width, p->height);
    if (p->numRaysPerPixel < 0) return fail(c, -2, "numRaysPerPixel < 0");
    if (p->rngMode != RT_RNG_PCG && p->rngMode != RT_RNG_PHILOX) return fail(c, -2, "unknown rngMode %d", p->rngMode);
    if (p->intersectMode != RT_INTERSECT_FLAT_CHUNKS && p->intersectMode != RT_INTERSECT_BRUTE) return fail(c, -2, "unknown intersectMode %d", p->intersectMode);
    // a moved camera keeps the previous frame's tile order and kernel choice as predictors; the next launch re-measures the costs
    if (!c->have_params || std::memcmp(&c->params, p, sizeof *p) != 0) c->tile_order_stale = true;
    if (c->have_params && c->params.rngMode != p->rngMode) c->auto_choice = -1;      // the kernels' relative speed depends on the RNG
    c->params = *p; c->have_params = true;
    return 0;
}

int rt_upload_spheres(rt_ctx* c, const rt_sphere* s, int n)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n < 0 || (n > 0 && !s)) return fail(c, -2, "bad sphere upload (n=%d)", n);
    c->h_spheres.assign(s, s + n); c->scene_dirty = true;
    return 0;
}
int rt_upload_triangles(rt_ctx* c, const rt_triangle* t, int n)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n < 0 || (n > 0 && !t)) return fail(c, -2, "bad triangle upload (n=%d)", n);
    // option "device_geometry": tris may lie in device memory.  Everything is checked before anything changes
    const int dev = (c->opt_device_geometry && n > 0) ? device_of_ptr(t) : -1;
    if (dev >= 0) {
        if (n > (1 << 28)) return fail(c, -3, "too many triangles (%d)", n);
        if (dev != c->device) return fail(c, -2, "rt_upload_triangles: tris lies in memory of device %d, the context is on device %d", dev, c->device);
        if ((uintptr_t)t % 4 != 0) return fail(c, -2, "rt_upload_triangles: the device pointer is not 4-byte aligned");
        RT_HIP(c, hipSetDevice(c->device));
        // new corners for the tree that stands (same count, built from resident triangles, nothing else uploaded or set since): it is
        // updated in place by the next frame or query.  Anything else is a new scene
        const bool deformation = !c->scene_dirty && !c->geom_local && c->tree_resident && (size_t)n == c->n_tris;
        if (!deformation && c->d_raw_tris.cap < (size_t)n * 18) RT_HIP(c, hipStreamSynchronize(c->stream));   // (the buffer is replaced: nothing may still read it)
        RT_HIP(c, c->d_raw_tris.ensure((size_t)n * 18));
        RT_HIP(c, hipMemcpyAsync(c->d_raw_tris.p, t, (size_t)n * sizeof(rt_triangle), hipMemcpyDeviceToDevice, c->stream));
        c->h_tris.clear(); c->h_tris.shrink_to_fit();
        c->tris_resident = true; c->n_resident = (size_t)n; c->geom_local = false;
        if (deformation) c->deform_pending = true;
        else c->scene_dirty = true;
        return 0;
    }
    c->h_tris.assign(t, t + n); c->scene_dirty = true; c->geom_local = false;
    c->tris_resident = false; c->n_resident = 0; c->deform_pending = false;
    return 0;
}
int rt_upload_meshinfo(rt_ctx* c, const rt_meshinfo* m, int n)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n < 0 || (n > 0 && !m)) return fail(c, -2, "bad meshinfo upload (n=%d)", n);
    c->h_mesh.assign(m, m + n); c->scene_dirty = true; c->geom_local = false;
    return 0;
}

int rt_upload_local_meshes(rt_ctx* c, const rt_triangle* tris, int n_tris, const rt_local_chunk* chunks, int n_chunks, int n_meshes)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n_tris < 0 || n_chunks < 0 || n_meshes < 0 || (n_tris > 0 && !tris) || (n_chunks > 0 && !chunks)) return fail(c, -2, "bad local mesh upload");
    if (n_tris > (1 << 28)) return fail(c, -3, "too many triangles (%d)", n_tris);
    std::vector<uint8_t> seen(n_tris, 0);
    std::vector<float> radius(n_meshes, 0.f);
    for (int m = 0; m < n_chunks; ++m) {
        const rt_local_chunk& ch = chunks[m];
        if ((uint64_t)ch.firstTriangleIndex + ch.numTriangles > (uint64_t)n_tris) return fail(c, -4, "chunk %d addresses triangles beyond the %d uploaded", m, n_tris);
        if (ch.meshIndex >= (uint32_t)n_meshes) return fail(c, -4, "chunk %d refers to mesh %u of %d", m, ch.meshIndex, n_meshes);
        for (uint32_t i = 0; i < ch.numTriangles; ++i) {
            uint8_t& s = seen[ch.firstTriangleIndex + i];
            if (s) return fail(c, -5, "triangle %u is referenced by more than one chunk", ch.firstTriangleIndex + i);
            s = 1;
            const float* p = tris[ch.firstTriangleIndex + i].posA;
            for (int k = 0; k < 9; ++k) radius[ch.meshIndex] = std::max(radius[ch.meshIndex], std::fabs(p[k]));
        }
    }
    for (int t = 0; t < n_tris; ++t) if (!seen[t]) return fail(c, -5, "triangle %d belongs to no chunk", t);
    for (float& r : radius) r *= 1.7320508f;
    c->h_local_tris.assign(tris, tris + n_tris); c->h_lchunks.assign(chunks, chunks + n_chunks);
    c->mesh_radius = radius; c->n_meshes = n_meshes;
    c->geom_local = true; c->scene_dirty = true;
    c->tris_resident = false; c->n_resident = 0; c->tree_resident = false; c->deform_pending = false;     // (d_raw_tris becomes this pipeline's output)
    return 0;
}

int rt_set_mesh_transforms(rt_ctx* c, const rt_mesh_transform* xf, int n_meshes)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n_meshes < 0 || (n_meshes > 0 && !xf)) return fail(c, -2, "bad transform upload");
    if (c->geom_local && n_meshes != c->n_meshes) return fail(c, -2, "%d transforms for %d meshes", n_meshes, c->n_meshes);
    c->h_xf.assign(xf, xf + n_meshes);
    c->xf_dirty = true;
    return 0;
}

int rt_read_world_geometry(rt_ctx* c, rt_triangle* tris_out, int n_tris, rt_meshinfo* mi_out, int n_chunks)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!c->geom_local) return fail(c, -2, "no local meshes uploaded");
    if (!c->have_params) return fail(c, -2, "rt_set_params has not been called");
    if (n_tris != (int)c->h_local_tris.size() || n_chunks != (int)c->h_lchunks.size()) return fail(c, -2, "size mismatch");
    RT_HIP(c, hipSetDevice(c->device));
    { int r = prepare_scene(c); if (r) return r; }     // (a pass for a wider padding refits node boxes only: the world triangles and chunk boxes stay)
    if (n_tris) RT_HIP(c, hipMemcpy(tris_out, c->d_raw_tris.p, (size_t)n_tris * sizeof(rt_triangle), hipMemcpyDeviceToHost));
    std::vector<float4> box(2 * (size_t)n_chunks);
    if (n_chunks) RT_HIP(c, hipMemcpy(box.data(), c->d_chunk_box.p, box.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (int m = 0; m < n_chunks; ++m) {
        const rt_local_chunk& ch = c->h_lchunks[m];
        rt_meshinfo& mi = mi_out[m];
        mi.firstTriangleIndex = ch.firstTriangleIndex; mi.numTriangles = ch.numTriangles; mi.material = ch.material;
        mi.boundsMin[0] = box[2 * m].x; mi.boundsMin[1] = box[2 * m].y; mi.boundsMin[2] = box[2 * m].z;
        mi.boundsMax[0] = box[2 * m + 1].x; mi.boundsMax[1] = box[2 * m + 1].y; mi.boundsMax[2] = box[2 * m + 1].z;
    }
    return 0;
}

int rt_set_option(rt_ctx* c, const char* name, int value)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!name) return fail(c, -2, "null option name");
    if (!std::strcmp(name, "kernel")) {
        if (value < -1 || value > 1) return fail(c, -2, "kernel must be -1 (auto), 0 (k_trace) or 1 (k_stream)");
        c->opt_kernel = value;
    }
    else if (!std::strcmp(name, "shade_threshold")) { if (value < 1 || value > 64) return fail(c, -2, "shade_threshold must be in [1,64]"); c->opt_shade_threshold = value; }
    else if (!std::strcmp(name, "stream_stack")) { if (value != 0 && (value < 4 || value > 128)) return fail(c, -2, "stream_stack must be 0 (automatic) or in [4,128]"); c->opt_stream_stack = value; }
    else if (!std::strcmp(name, "lds_stack")) { if (value < 0 || value > 64) return fail(c, -2, "lds_stack must be in [0,64]"); c->opt_lds_stack = value; }
    else if (!std::strcmp(name, "bvh_bins")) { if (value < 2 || value > 128) return fail(c, -2, "bvh_bins must be in [2,128]"); if (value != c->opt_bvh_bins) c->scene_dirty = true; c->opt_bvh_bins = value; }
    else if (!std::strcmp(name, "bvh_reinsert")) { if (value < 0 || value > 16) return fail(c, -2, "bvh_reinsert must be in [0,16]"); if (value != c->opt_bvh_reinsert) c->scene_dirty = true; c->opt_bvh_reinsert = value; }
    else if (!std::strcmp(name, "bvh_cost_exp")) { if (value < 10 || value > 300) return fail(c, -2, "bvh_cost_exp must be in [10,300] (percent)"); if (value != c->opt_bvh_cost_exp) c->scene_dirty = true; c->opt_bvh_cost_exp = value; }
    else if (!std::strcmp(name, "max_leaf")) { if (value < 1 || value > rtbvh::kMaxLeaf) return fail(c, -2, "max_leaf must be in [1,4]"); if (value != c->opt_max_leaf) c->scene_dirty = true; c->opt_max_leaf = value; }
    else if (!std::strcmp(name, "bvh_collapse")) { if (value < 0 || value > 2) return fail(c, -2, "bvh_collapse must be 0 (greedy), 1 (cost-driven, leaves formed by the collapse) or 2 (cost-driven over the split search's leaves)"); if (value != c->opt_bvh_collapse) c->scene_dirty = true; c->opt_bvh_collapse = value; }
    else if (!std::strcmp(name, "bvh_node_cost")) { if (value < 1 || value > 10000) return fail(c, -2, "bvh_node_cost must be in [1,10000] (percent of a triangle test)"); if (value != c->opt_bvh_node_cost) c->scene_dirty = true; c->opt_bvh_node_cost = value; }
    else if (!std::strcmp(name, "tile_w_log2")) { if (value < 0 || value > 6) return fail(c, -2, "tile_w_log2 must be in [0,6]"); c->opt_tile_w_log2 = value; }
    else if (!std::strcmp(name, "tile_lpt")) { c->opt_tile_lpt = value ? 1 : 0; c->tile_order_valid = false; }
    else if (!std::strcmp(name, "frame_batch")) { if (value < 0 || value > 1024) return fail(c, -2, "frame_batch must be in [0,1024]"); c->opt_frame_batch = value; }
    else if (!std::strcmp(name, "fetch_guide")) { if (value < 1 || value > 64) return fail(c, -2, "fetch_guide must be in [1,64]"); c->opt_fetch_guide = value; }
    else if (!std::strcmp(name, "fetch_guide_philox")) { if (value < 1 || value > 64) return fail(c, -2, "fetch_guide_philox must be in [1,64]"); c->opt_fetch_guide_philox = value; }
    else if (!std::strcmp(name, "tiles_per_fetch")) { if (value < 1 || value > 64) return fail(c, -2, "tiles_per_fetch must be in [1,64]"); c->opt_tiles_per_fetch = value; }
    else if (!std::strcmp(name, "node_min")) { if (value < 1 || value > 64) return fail(c, -2, "node_min must be in [1,64]"); c->opt_node_min = value; }
    else if (!std::strcmp(name, "tile_sync")) c->opt_tile_sync = value ? 1 : 0;
    else if (!std::strcmp(name, "compact_nodes")) c->opt_compact_nodes = value ? 1 : 0;
    else if (!std::strcmp(name, "device_bvh")) { if (value < -1 || value > 1) return fail(c, -2, "device_bvh must be -1 (automatic), 0 or 1"); if (value != c->opt_device_bvh) c->scene_dirty = true; c->opt_device_bvh = value; }
    else if (!std::strcmp(name, "bvh_radius")) { if (value == 0 || value < -rtgb::kMaxRadius || value > rtgb::kMaxRadius) return fail(c, -2, "bvh_radius must be in [1,64] (negative: the same radius in every round)"); if (value != c->opt_bvh_radius) c->scene_dirty = true; c->opt_bvh_radius = value; }
    else if (!std::strcmp(name, "device_geometry")) { if (value != 0 && value != 1) return fail(c, -2, "device_geometry must be 0 or 1"); c->opt_device_geometry = value; }
    else if (!std::strcmp(name, "peer_copies")) { if (value != 0 && value != 1) return fail(c, -2, "peer_copies must be 0 or 1"); c->opt_peer_copies = value; }
    else if (!std::strcmp(name, "bvh_treelet_ratio")) { if (value < 2 || value > 64) return fail(c, -2, "bvh_treelet_ratio must be in [2,64]"); if (value != c->opt_bvh_treelet_ratio) c->scene_dirty = true; c->opt_bvh_treelet_ratio = value; }
    else if (!std::strcmp(name, "bvh_treelet_isolate")) { if (value < 0 || value > 1) return fail(c, -2, "bvh_treelet_isolate must be 0 or 1"); if (value != c->opt_bvh_treelet_isolate) c->scene_dirty = true; c->opt_bvh_treelet_isolate = value; }
    else if (!std::strcmp(name, "bvh_treelet_first")) { if (value < 1 || value > 4096) return fail(c, -2, "bvh_treelet_first must be in [1,4096]"); if (value != c->opt_bvh_treelet_first) c->scene_dirty = true; c->opt_bvh_treelet_first = value; }
    else if (!std::strcmp(name, "bvh_treelets")) { if (value < 0 || value > 16) return fail(c, -2, "bvh_treelets must be in [0,16] (passes)"); if (value != c->opt_bvh_treelets) c->scene_dirty = true; c->opt_bvh_treelets = value; }
    else if (!std::strcmp(name, "bvh_top")) { if (value < 0 || value > (1 << 20)) return fail(c, -2, "bvh_top must be in [0,1048576] (0 = the device's clustering builds the whole tree)"); if (value != c->opt_bvh_top) c->scene_dirty = true; c->opt_bvh_top = value; }
    else if (!std::strcmp(name, "rebuild_percent")) { if (value < 0 || value > 100000) return fail(c, -2, "rebuild_percent must be in [0,100000] (0 = never rebuild)"); c->opt_rebuild_percent = value; }
    else if (!std::strcmp(name, "stream_tile")) { if (value != 0 && value != 2 && value != 4) return fail(c, -2, "stream_tile must be 0 (8x8 pixels x 1 frame), 2 (4x4 x 4 frames) or 4 (2x2 x 16 frames)"); c->opt_stream_tile = value; }
    else if (!std::strcmp(name, "full_sort")) c->opt_full_sort = value ? 1 : 0;
    else if (!std::strcmp(name, "primary_lists")) { if (value != 0 && value != 1) return fail(c, -2, "primary_lists must be 0 or 1"); c->opt_primary_lists = value; }
    else if (!std::strcmp(name, "queue_depth")) { if (value < 1 || value > 256) return fail(c, -2, "queue_depth must be in [1,256]"); c->opt_queue_depth = value; }
    else if (!std::strcmp(name, "queue_linger_us")) { if (value < 0 || value > 1000000) return fail(c, -2, "queue_linger_us must be in [0,1000000]"); c->opt_queue_linger_us = value; }
    else if (!std::strcmp(name, "gather_slice")) { if (value < 1 || value > kQuerySlice) return fail(c, -2, "gather_slice must be in [1,%d] (points per launch)", kQuerySlice); c->opt_gather_slice = value; }
    else if (!std::strcmp(name, "visibility_slice")) { if (value < 1 || value > kQuerySlice) return fail(c, -2, "visibility_slice must be in [1,%d] (points per launch)", kQuerySlice); c->opt_visibility_slice = value; }
    else if (!std::strcmp(name, "closest_slice")) { if (value < 1 || value > kQuerySlice) return fail(c, -2, "closest_slice must be in [1,%d] (points per launch)", kQuerySlice); c->opt_closest_slice = value; }
    else if (!std::strcmp(name, "hits_slice")) { if (value < 1 || value > kQuerySlice) return fail(c, -2, "hits_slice must be in [1,%d] (rays per launch)", kQuerySlice); c->opt_hits_slice = value; }
    else if (!std::strcmp(name, "closest_count")) { if (value != 0 && value != 1) return fail(c, -2, "closest_count must be 0 or 1"); c->opt_closest_count = value; }
    else if (!std::strcmp(name, "closest_k")) { if (value < 1 || value > RT_HITS_MAX) return fail(c, -2, "closest_k must be in [1,%d] (records per point)", RT_HITS_MAX); c->opt_closest_k = value; }
    else if (!std::strcmp(name, "closest_all")) { if (value != 0 && value != 1) return fail(c, -2, "closest_all must be 0 or 1"); c->opt_closest_all = value; }
    else if (!std::strcmp(name, "closest_box")) { if (value != 0 && value != 1) return fail(c, -2, "closest_box must be 0 or 1"); c->opt_closest_box = value; }
    else if (!std::strcmp(name, "sweep")) { if (value != 0 && value != 1) return fail(c, -2, "sweep must be 0 or 1"); c->opt_sweep = value; }
    else if (!std::strcmp(name, "radiance_slice")) { if (value < 1 || value > kQuerySlice) return fail(c, -2, "radiance_slice must be in [1,%d] (rays per launch)", kQuerySlice); c->opt_radiance_slice = value; }
    else if (!std::strcmp(name, "blocks_per_cu")) { if (value < 0) return fail(c, -2, "blocks_per_cu must be >= 0"); c->opt_blocks_per_cu = value; }
    else return fail(c, -2, "unknown option '%s'", name);
    return 0;
}

int rt_set_rows(rt_ctx* c, int row0, int nrows)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (row0 < 0 || nrows < 0) return fail(c, -2, "bad row strip (%d,%d)", row0, nrows);
    c->row0 = row0; c->nrows = nrows; c->band_stride = 0;
    return 0;
}

int rt_set_bands(rt_ctx* c, int first_band, int band_stride)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (first_band < 0 || band_stride < 1 || first_band >= band_stride) return fail(c, -2, "bad band pattern (%d,%d)", first_band, band_stride);
    c->band_first = first_band; c->band_stride = band_stride;
    return 0;
}

int rt_render_frame(rt_ctx* c, int frame_index) { if (!c) return -1; RT_SETTLE(c); return launch_frames(c, frame_index, 1, Variant::Fast); }
int rt_render(rt_ctx* c, int first_frame, int n_frames) { if (!c) return -1; RT_SETTLE(c); return launch_frames(c, first_frame, n_frames, Variant::Fast); }
int rt_render_counting(rt_ctx* c, int first_frame, int n_frames) { if (!c) return -1; RT_SETTLE(c); return launch_frames(c, first_frame, n_frames, Variant::Counting); }
int rt_render_frame_flat(rt_ctx* c, int frame_index) { if (!c) return -1; RT_SETTLE(c); return launch_frames(c, frame_index, 1, Variant::Flat); }

int rt_render_params(rt_ctx* c, int first_frame, int n_frames, const rt_params* params)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (n_frames < 0) return fail(c, -2, "n_frames < 0");
    if (n_frames == 0) return 0;
    if (!params) return fail(c, -2, "null params");
    if (const int f = other_settings(params, n_frames)) return fail(c, -2, "rt_render_params: entry %d differs from entry 0 outside the camera fields", f);
    if (!c->have_params || !same_settings(c->params, params[0])) { const int r = rt_set_params(c, &params[0]); if (r) return r; }
    return launch_run(c, first_frame, n_frames, params);
}

// Queued submission.  rt_submit_frame returns at once; a worker thread of the library traces the queued frames in launches of whatever
// has queued up while the previous launch ran (consecutive frame indices share a launch: frame-interleaved work items, one launch tail)
// and accumulates them in submission order — the image equals rt_render's over the same frames, bit for bit.
int rt_submit_frame(rt_ctx* c, int frame_index)
{
    if (!c) return -1;
    if (!c->have_params) { RT_SETTLE(c); return fail(c, -2, "rt_set_params has not been called"); }
    {
        std::lock_guard<std::mutex> lk(c->q_mu);
        if (c->q_rc) return c->q_rc;                    // a queued launch failed: rt_wait (or any other call) reports it
        queue_push(c, frame_index, queue_tail(c));
    }
    c->q_cv.notify_one();
    return 0;
}
int rt_submit_frame_params(rt_ctx* c, int frame_index, const rt_params* p)
{
    if (!c) return -1;
    if (!p) { RT_SETTLE(c); return fail(c, -2, "null params"); }
    bool new_settings;
    {
        std::lock_guard<std::mutex> lk(c->q_mu);
        if (c->q_rc) return c->q_rc;
        new_settings = !c->have_params || !same_settings(queue_tail(c), *p);
    }
    if (new_settings) { const int r = rt_set_params(c, p); if (r) return r; }      // settles the queue first; a moved camera does not wait
    {
        std::lock_guard<std::mutex> lk(c->q_mu);
        queue_push(c, frame_index, *p);
    }
    c->q_cv.notify_one();
    return 0;
}
int rt_wait(rt_ctx* c) { if (!c) return -1; RT_SETTLE(c); return 0; }

int rt_reset_accum(rt_ctx* c)
{
    if (!c) return -1;
    RT_SETTLE(c);
    RT_HIP(c, hipSetDevice(c->device));
    if (c->target.pixels()) {
        RT_HIP(c, hipMemsetAsync(c->d_accum.p, 0, c->target.pixels() * sizeof(float4), c->stream));
        RT_HIP(c, hipMemsetAsync(c->d_frame.p, 0, c->target.pixels() * sizeof(float4), c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->stats.numRenderedFrames = 0; c->stats.totalKernelMs = 0; c->stats.queuedLaunches = 0;
    return 0;
}

int rt_write_accum(rt_ctx* c, const float* rgba, size_t n_floats, int frames_rendered)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!rgba && n_floats) return fail(c, -2, "null source");
    if (frames_rendered < 0) return fail(c, -2, "frames_rendered < 0");
    if (!c->have_params) return fail(c, -2, "rt_set_params has not been called");
    RT_HIP(c, hipSetDevice(c->device));
    { int r = ensure_targets(c); if (r) return r; }
    if (n_floats != c->target.pixels() * 4) return fail(c, -2, "expected %zu floats (rows*width*4), got %zu", c->target.pixels() * 4, n_floats);
    if (n_floats) {
        RT_HIP(c, hipMemcpyAsync(c->d_accum.p, rgba, n_floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->stats.numRenderedFrames = frames_rendered;
    return 0;
}

int rt_read_accum(rt_ctx* c, float* rgba, size_t n) { if (!c) return -1; RT_SETTLE(c); return read_target(c, true, rgba, n, false); }
int rt_read_last_frame(rt_ctx* c, float* rgba, size_t n) { if (!c) return -1; RT_SETTLE(c); return read_target(c, false, rgba, n, false); }
int rt_copy_accum_to_device(rt_ctx* c, void* dst, size_t n) { if (!c) return -1; RT_SETTLE(c); return read_target(c, true, (float*)dst, n, true); }

int rt_read_display(rt_ctx* c, uint32_t* rgba8, size_t n_pixels)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!rgba8 && n_pixels) return fail(c, -2, "null destination");
    if (c->have_params) { int r = ensure_targets(c); if (r) return r; }
    if (n_pixels != c->target.pixels()) return fail(c, -2, "expected %zu pixels (rows*width), got %zu", c->target.pixels(), n_pixels);
    if (!n_pixels) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    float ms = 0.f;
    RT_HIP(c, display_plane(c, c->d_accum.p, c->d_display, rgba8, n_pixels, &ms));
    c->stats.lastDisplayMs = ms;
    return 0;
}

int rt_read_bvh(rt_ctx* c, void* nodes_f32, void* nodes_f16, size_t n_nodes)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (c->scene_dirty) return fail(c, -2, "the scene has not been built yet (render a frame first)");
    if (n_nodes != c->n_nodes) return fail(c, -2, "expected %zu nodes, got %zu", c->n_nodes, n_nodes);
    if (!n_nodes) return 0;
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (nodes_f32) RT_HIP(c, hipMemcpy(nodes_f32, c->d_nodes.p, n_nodes * 128, hipMemcpyDeviceToHost));
    if (nodes_f16) RT_HIP(c, hipMemcpy(nodes_f16, c->d_nodes_h.p, n_nodes * 128, hipMemcpyDeviceToHost));
    return 0;
}

int rt_read_bvh_order(rt_ctx* c, uint32_t* order, size_t n)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (c->scene_dirty) return fail(c, -2, "the scene has not been built yet (render a frame first)");
    const size_t have = c->n_nodes ? c->d_order.used : 0;
    if (n != have) return fail(c, -2, "expected %zu triangles, got %zu", have, n);
    if (!n) return 0;
    if (!order) return fail(c, -2, "null destination");
    RT_HIP(c, hipSetDevice(c->device));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    RT_HIP(c, hipMemcpy(order, c->d_order.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int rt_trace_rays(rt_ctx* c, const rt_ray* rays, int n, rt_hit* hits) { return query_entry(c, trace_rays_call, "rt_trace_rays", false, rays, n, nullptr, hits); }
int rt_occluded(rt_ctx* c, const rt_ray* rays, int n, uint8_t* occluded) { return query_entry(c, occluded_call, "rt_occluded", false, rays, n, nullptr, occluded); }
int rt_trace_rays_device(rt_ctx* c, const void* rays, int n, void* hits) { return query_entry(c, trace_rays_call, "rt_trace_rays_device", true, rays, n, nullptr, hits); }
int rt_occluded_device(rt_ctx* c, const void* rays, int n, void* occluded) { return query_entry(c, occluded_call, "rt_occluded_device", true, rays, n, nullptr, occluded); }
int rt_trace_radiance(rt_ctx* c, const rt_ray* rays, int n, const rt_radiance_params* params, float* rgba) { return query_entry(c, radiance_call, "rt_trace_radiance", false, rays, n, params, rgba); }
int rt_trace_radiance_device(rt_ctx* c, const void* rays, int n, const rt_radiance_params* params, void* rgba) { return query_entry(c, radiance_call, "rt_trace_radiance_device", true, rays, n, params, rgba); }
int rt_gather(rt_ctx* c, const rt_ray* points, int n, const rt_gather_params* params, float* out) { return query_entry(c, gather_call, "rt_gather", false, points, n, params, out); }
int rt_gather_device(rt_ctx* c, const void* points, int n, const rt_gather_params* params, void* out) { return query_entry(c, gather_call, "rt_gather_device", true, points, n, params, out); }
int rt_visibility(rt_ctx* c, const rt_ray* points, int n, const rt_visibility_params* params, float* out) { return query_entry(c, visibility_call, "rt_visibility", false, points, n, params, out); }
int rt_visibility_device(rt_ctx* c, const void* points, int n, const rt_visibility_params* params, void* out) { return query_entry(c, visibility_call, "rt_visibility_device", true, points, n, params, out); }
int rt_closest_points(rt_ctx* c, const rt_ray* points, int n, rt_closest* out) { return query_entry(c, closest_call, "rt_closest_points", false, points, n, nullptr, out); }
int rt_closest_points_device(rt_ctx* c, const void* points, int n, void* out) { return query_entry(c, closest_call, "rt_closest_points_device", true, points, n, nullptr, out); }
// The counts of a counting call are fetched here, once: the call's one wait when it came through the device entry
int rt_get_closest_info(rt_ctx* c, rt_closest_info* out)
{
    if (!c || !out) return -1;
    if (c->closest_counts_pending) {
        RT_HIP(c, hipSetDevice(c->device));
        RT_HIP(c, hipMemcpyAsync(c->closest_counts, c->d_closest_counts.p, sizeof c->closest_counts, hipMemcpyDeviceToHost, c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
        c->closest_counts_pending = false;
    }
    const rt_gather_info& g = c->query_info[kClosest];
    *out = rt_closest_info{};
    out->calls = g.calls; out->lastKernelMs = g.lastKernelMs; out->totalKernelMs = g.totalKernelMs;
    out->lastNodeSteps = c->closest_counts[0]; out->lastPrimTests = c->closest_counts[1];
    return 0;
}
int rt_trace_hits(rt_ctx* c, const rt_ray* rays, int n, const rt_hits_params* params, rt_multihit* out) { return query_entry(c, hits_call, "rt_trace_hits", false, rays, n, params, out); }
int rt_trace_hits_device(rt_ctx* c, const void* rays, int n, const rt_hits_params* params, void* out) { return query_entry(c, hits_call, "rt_trace_hits_device", true, rays, n, params, out); }
int rt_get_hits_info(rt_ctx* c, rt_hits_info* out)
{
    if (!c || !out) return -1;
    const rt_gather_info& g = c->query_info[kHits];
    *out = rt_hits_info{};
    out->calls = g.calls; out->lastKernelMs = g.lastKernelMs; out->totalKernelMs = g.totalKernelMs;
    out->lastMaxHits = c->hits_last.maxHits; out->lastMode = c->hits_last.mode; out->lastCountAll = c->hits_last.countAll;
    return 0;
}
// (the three info records are one layout, checked where QueryFamily is declared)
int rt_get_gather_info(rt_ctx* c, rt_gather_info* out)
{
    if (!c || !out) return -1;
    *out = c->query_info[kGather];
    return 0;
}
int rt_get_visibility_info(rt_ctx* c, rt_visibility_info* out)
{
    if (!c || !out) return -1;
    std::memcpy(out, &c->query_info[kVisibility], sizeof *out);
    return 0;
}
int rt_get_radiance_info(rt_ctx* c, rt_radiance_info* out)
{
    if (!c) return -1;
    if (!out) return fail(c, -2, "null out");
    std::memcpy(out, &c->query_info[kRadiance], sizeof *out);
    return 0;
}

int rt_render_aov(rt_ctx* c, int first_frame, int n_frames) { return c ? render_aov(c, first_frame, n_frames) : -1; }
int rt_read_aov(rt_ctx* c, int which, float* rgba, size_t n) { return c ? read_aov(c, which, rgba, n, false) : -1; }
int rt_copy_aov_to_device(rt_ctx* c, int which, void* dst, size_t n) { return c ? read_aov(c, which, dst, n, true) : -1; }
int rt_reset_aov(rt_ctx* c)
{
    if (!c) return -1;
    RT_SETTLE(c);
    RT_HIP(c, hipSetDevice(c->device));
    if (c->aov.pixels()) {
        for (DevBuf<float4>& b : c->d_aov) RT_HIP(c, hipMemsetAsync(b.p, 0, c->aov.pixels() * sizeof(float4), c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->aov_info.framesAccumulated = 0; c->aov_info.totalKernelMs = 0;
    return 0;
}
int rt_get_aov_info(rt_ctx* c, rt_aov_info* out) { return c ? read_info(c, c->aov_info, out) : -1; }

int rt_denoise(rt_ctx* c, const rt_denoise_params* params) { return denoise_call(c, { "rt_denoise", "rt_multi_denoise" }, false, params); }
int rt_read_denoised(rt_ctx* c, float* rgba, size_t n) { return read_own(c, OwnPlane::Denoised, rgba, n, false); }
int rt_copy_denoised_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Denoised, dst, n, true); }
int rt_read_denoised_display(rt_ctx* c, uint32_t* rgba8, size_t n_pixels)
{
    if (!c) return -1;
    RT_SETTLE(c);
    return read_filter_display(c, c, c->dn, "rt_denoise", c->dn.out.p, c->d_display, rgba8, n_pixels);
}
int rt_get_denoise_info(rt_ctx* c, rt_denoise_info* out) { return c ? read_info(c, c->dn.info, out) : -1; }

int rt_denoise_variance(rt_ctx* c, const rt_vdenoise_params* params)
{
    return denoise_variance_call(c, { "rt_denoise_variance", "rt_multi_denoise_variance", "source 1, and " }, params);
}
int rt_read_variance(rt_ctx* c, float* var, size_t n) { return read_own(c, OwnPlane::Variance, var, n, false); }
int rt_copy_variance_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Variance, dst, n, true); }
int rt_get_vdenoise_info(rt_ctx* c, rt_vdenoise_info* out) { return c ? read_info(c, c->vd.info, out) : -1; }

int rt_temporal(rt_ctx* c, const rt_temporal_params* params) { return temporal_call(c, { "rt_temporal", "rt_multi_temporal" }, params); }
int rt_denoise_temporal(rt_ctx* c, const rt_denoise_params* params)
{
    return denoise_call(c, { "rt_denoise_temporal", "rt_multi_temporal" }, true, params);
}
int rt_reset_temporal(rt_ctx* c)
{
    if (!c) return -1;
    RT_SETTLE(c);
    c->tp.reset();
    return 0;
}
int rt_read_temporal(rt_ctx* c, float* rgba, size_t n) { return read_own(c, OwnPlane::Temporal, rgba, n, false); }
int rt_read_temporal_history(rt_ctx* c, float* hist, size_t n) { return read_own(c, OwnPlane::History, hist, n, false); }
int rt_copy_temporal_to_device(rt_ctx* c, void* dst, size_t n) { return read_own(c, OwnPlane::Temporal, dst, n, true); }
int rt_read_temporal_display(rt_ctx* c, uint32_t* rgba8, size_t n_pixels)
{
    if (!c) return -1;
    RT_SETTLE(c);
    return read_filter_display(c, c, c->tp, "rt_temporal", c->tp.t[c->tp.cur].p, c->d_display, rgba8, n_pixels);
}
int rt_get_temporal_info(rt_ctx* c, rt_temporal_info* out) { return c ? read_info(c, c->tp.info, out) : -1; }

int rt_get_stats(rt_ctx* c, rt_stats* out)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!out) return fail(c, -2, "null stats");
    *out = c->stats;
    return 0;
}

} // extern "C"

// ---- several devices behind one handle: frames tile across the GPUs of a node -------------------------------------------
// The path shards into independent pixels (seeds use global pixel coordinates, RayTracing.shader:360-362; accumulation is per
// pixel), so every device holds the whole scene, renders the 8-row bands b with b % N == its rank for all frames, and one
// gather at the end of rt_multi_render brings the strips to the first device: N - 1 peer copies (xGMI point-to-point, each over
// its own link on a fully connected node) and a row scatter.  No other exchange exists on the path.
struct rt_multi : ErrOwner {
    std::vector<rt_ctx*> ctx;
    int width = 0, height = 0;
    bool have_params = false;
    DevBuf<float4> d_image, d_staging;          // on the first context's device: the assembled image, the incoming strips
    DevBuf<uint32_t> d_display;                 // ... and its sRGB8 form (rt_multi_read_display)
    DevBuf<float4> d_aov_image;                 // ... the assembled feature plane of the last rt_multi_read_aov
    DevBuf<float4> d_dn_albedo, d_dn_guide;     // ... both assembled feature planes of the last rt_multi_denoise
    DenoisePlanes dn;                           // ... its work planes and the denoised plane
    VariancePlane vd;                           // ... var_0 of the last rt_multi_denoise_variance
    TemporalPlanes tp;                          // ... the state of rt_multi_temporal
    std::vector<hipEvent_t> ev_strip;           // per context: its strip has arrived on the first device (recorded on the SOURCE context's stream)
    int max_rows = 0;
    double lastGatherMs = 0, lastSetupMs = 0;
    bool scene_dirty = true;                    // the first context holds an upload the others have not received yet
    std::vector<int> peer;                      // per context: 1 = the first context's device reads its memory directly (peer access on), 0 = staged by the runtime
};

namespace {

template <class Fn> int for_each_ctx(rt_multi* m, const char* what, Fn f)
{
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        const int r = f(m->ctx[i]);
        if (r) return fail(m, r, "%s on context %zu: %s", what, i, rt_last_error(m->ctx[i]));
    }
    return 0;
}

// fn(i) for every context at once — one host thread per context (a context is single-threaded, the contexts are independent), context
// 0 on the caller's; the first context that failed is reported as a failure of `what`
template <class Fn> int on_every_context(rt_multi* m, const char* what, Fn fn)
{
    const int N = (int)m->ctx.size();
    std::vector<int> rc(N, 0);
    {
        std::vector<std::thread> th;
        for (int i = 1; i < N; ++i) th.emplace_back([&, i]() { rc[i] = fn(i); });
        rc[0] = fn(0);
        for (std::thread& t : th) t.join();
    }
    for (int i = 0; i < N; ++i) if (rc[i]) return fail(m, rc[i], "%s on context %d: %s", what, i, rt_last_error(m->ctx[i]));
    return 0;
}

// copy_plane's counterpart for the handle's planes that are assembled on demand (rt_multi_read_aov, rt_multi_read_accum): a whole-image
// plane on the first device -> the host.  source(src) says where the plane is, assembling it first if need be; it runs once the size is
// known to be right and not zero
template <class Source> int read_image(rt_multi* m, size_t expect_floats, float* dst, size_t n_floats, Source source)
{
    if (n_floats != expect_floats) return fail(m, -2, "expected %zu floats (height*width*4), got %zu", expect_floats, n_floats);
    if (!n_floats) return 0;
    const float4* src = nullptr;
    { int r = source(src); if (r) return r; }
    RT_HIP(m, hipSetDevice(m->ctx[0]->device));
    RT_HIP(m, hipMemcpy(dst, src, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// rows of rank r (bands r, r + N, ...) from its strip to their places in the image
__global__ __launch_bounds__(256) void k_scatter_bands(const float4* __restrict__ strip, float4* __restrict__ image, int W, int H, int rank, int N)
{
    const size_t n = (size_t)W * 8;
    int local_band = blockIdx.y;
    const int y0 = (rank + local_band * N) * 8;
    if (y0 >= H) return;
    const int rows = min(8, H - y0);
    const float4* src = strip + (size_t)local_band * n;
    float4* dst = image + (size_t)y0 * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)rows * W; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

} // namespace

extern "C" {

rt_multi* rt_multi_create(const int* devices, int n_devices)
{
    if (n_devices < 1 || !devices) { fail(nullptr, -1, "rt_multi_create: no devices given"); return nullptr; }
    rt_multi* m = new rt_multi();
    for (int i = 0; i < n_devices; ++i) {
        rt_ctx* c = rt_create(devices[i]);
        if (!c) { const std::string e = g_create_error; rt_multi_destroy(m); g_create_error = e; return nullptr; }
        m->ctx.push_back(c);
    }
    // direct peer copies between the first device and the others where the hardware allows it; a refusal only means that the runtime
    // stages the copy (rt_multi_get_info reports which it is, per context)
    m->peer.assign(n_devices, 1);
    m->ev_strip.assign(n_devices, nullptr);
    for (int i = 1; i < n_devices; ++i) {
        (void)hipSetDevice(m->ctx[i]->device);
        if (hipEventCreateWithFlags(&m->ev_strip[i], hipEventDisableTiming) != hipSuccess) { fail(nullptr, -1, "rt_multi_create: event for context %d", i); rt_multi_destroy(m); return nullptr; }
    }
    for (int i = 1; i < n_devices; ++i)
        if (m->ctx[i]->device != m->ctx[0]->device) {
            int ok = 1;
            for (int dir = 0; dir < 2; ++dir) {
                const int a = dir ? m->ctx[i]->device : m->ctx[0]->device, b = dir ? m->ctx[0]->device : m->ctx[i]->device;
                int can = 0;
                (void)hipSetDevice(a);
                if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) { ok = 0; continue; }
                const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ok = 0;
            }
            (void)hipGetLastError();
            m->peer[i] = ok;
        }
    return m;
}

void rt_multi_destroy(rt_multi* m)
{
    if (!m) return;
    for (size_t i = 0; i < m->ev_strip.size() && i < m->ctx.size(); ++i)
        if (m->ev_strip[i]) { (void)hipSetDevice(m->ctx[i]->device); (void)hipEventDestroy(m->ev_strip[i]); }
    const int device0 = m->ctx.empty() ? -1 : m->ctx[0]->device;
    for (rt_ctx* c : m->ctx) rt_destroy(c);
    if (device0 >= 0) (void)hipSetDevice(device0);      // the handle's own planes live on the first context's device
    delete m;
}

const char* rt_multi_last_error(const rt_multi* m) { return m ? m->err.c_str() : g_create_error.c_str(); }
int rt_multi_count(const rt_multi* m) { return m ? (int)m->ctx.size() : 0; }
rt_ctx* rt_multi_context(rt_multi* m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }

int rt_multi_set_params(rt_multi* m, const rt_params* p)
{
    if (!m) return -1;
    if (!p) return fail(m, -2, "null params");
    const int N = (int)m->ctx.size();
    for (int i = 0; i < N; ++i) {
        int r = rt_set_params(m->ctx[i], p);
        if (!r) r = rt_set_bands(m->ctx[i], i, N);
        if (r) return fail(m, r, "rt_set_params on context %d: %s", i, rt_last_error(m->ctx[i]));
    }
    m->width = p->width; m->height = p->height; m->have_params = true;
    return 0;
}
// The three buffers go to the FIRST context only: it builds the scene once (re-layout + BVH) at the next rt_multi_render and the other
// contexts receive the built scene device to device (clone_scene) — one build and one host -> device upload per scene change, whatever N.
static int multi_upload(rt_multi* m, int r, const char* what)
{
    if (r) return fail(m, r, "%s on context 0: %s", what, rt_last_error(m->ctx[0]));
    m->scene_dirty = true;
    return 0;
}
int rt_multi_upload_spheres(rt_multi* m, const rt_sphere* s, int n)
{
    if (!m) return -1;
    // (a few records: every context takes them — with the geometry pipeline each context builds for itself, whichever upload comes first)
    const int r = for_each_ctx(m, "rt_upload_spheres", [&](rt_ctx* c) { return rt_upload_spheres(c, s, n); });
    if (!r && !m->ctx[0]->geom_local) m->scene_dirty = true;
    return r;
}
int rt_multi_upload_triangles(rt_multi* m, const rt_triangle* t, int n) { return m ? multi_upload(m, rt_upload_triangles(m->ctx[0], t, n), "rt_upload_triangles") : -1; }
int rt_multi_upload_meshinfo(rt_multi* m, const rt_meshinfo* mi, int n) { return m ? multi_upload(m, rt_upload_meshinfo(m->ctx[0], mi, n), "rt_upload_meshinfo") : -1; }
// On-device geometry pipeline behind the handle.  Every context receives the local meshes once and the poses (40 B per mesh) per frame and
// transforms, builds and refits ON ITS OWN DEVICE (the device build takes a few milliseconds): no geometry crosses xGMI per frame.
int rt_multi_upload_local_meshes(rt_multi* m, const rt_triangle* tris, int n_tris, const rt_local_chunk* chunks, int n_chunks, int n_meshes)
{
    if (!m) return -1;
    const int r = for_each_ctx(m, "rt_upload_local_meshes", [&](rt_ctx* c) { return rt_upload_local_meshes(c, tris, n_tris, chunks, n_chunks, n_meshes); });
    if (!r) m->scene_dirty = false;             // nothing to fan out: every context holds the upload itself
    return r;
}
int rt_multi_set_mesh_transforms(rt_multi* m, const rt_mesh_transform* xf, int n_meshes)
{
    return m ? for_each_ctx(m, "rt_set_mesh_transforms", [&](rt_ctx* c) { return rt_set_mesh_transforms(c, xf, n_meshes); }) : -1;
}
int rt_multi_set_option(rt_multi* m, const char* name, int value)
{
    if (!m) return -1;
    const int r = for_each_ctx(m, "rt_set_option", [&](rt_ctx* c) { return rt_set_option(c, name, value); });
    if (!r && m->ctx[0]->scene_dirty) m->scene_dirty = true;        // (a builder option: the first context rebuilds, the others receive the new tree)
    return r;
}
int rt_multi_reset_accum(rt_multi* m) { return m ? for_each_ctx(m, "rt_reset_accum", [&](rt_ctx* c) { return rt_reset_accum(c); }) : -1; }

} // extern "C"

namespace {
// Every context holds the scene: after an upload the first context builds it (build_root) and the others receive the result
template <class Fn> int multi_share_scene(rt_multi* m, Fn build_root)
{
    const int N = (int)m->ctx.size();
    bool stale = m->scene_dirty;
    for (rt_ctx* c : m->ctx) stale = stale || c->scene_dirty;       // (a builder option set through rt_multi_context(i), a context never filled)
    if (m->ctx[0]->geom_local) {
        // geometry pipeline: every context holds the local meshes and builds / refits on its own device, inside its rt_render below
        for (rt_ctx* c : m->ctx) if (!c->geom_local) return fail(m, -2, "rt_multi: some contexts hold local meshes and some do not (use the rt_multi_upload_* calls)");
        stale = false; m->scene_dirty = false;
    }
    if (stale) {
        // ---- scene change: the first context builds (one BVH build, one host -> device upload), the others receive the result
        const double t0 = now_ms();
        rt_ctx* root = m->ctx[0];
        { int r = build_root(root); if (r) return fail(m, r, "scene build on context 0: %s", rt_last_error(root)); }
        std::vector<int> rcs(N, 0);
        {
            std::vector<std::thread> th;
            for (int i = 1; i < N; ++i) th.emplace_back([&, i]() { rcs[i] = clone_scene(m->ctx[i], root); });
            for (std::thread& t : th) t.join();
        }
        for (int i = 1; i < N; ++i) if (rcs[i]) return fail(m, rcs[i], "scene transfer to context %d: %s", i, rt_last_error(m->ctx[i]));
        m->scene_dirty = false;
        m->lastSetupMs = now_ms() - t0;
    }
    return 0;
}

// The gather: every context's strip (strip(c): its device buffer of rows(c) rows) -> the first device, rows to their places in `image`
template <class Strip, class Rows> int gather_strips(rt_multi* m, DevBuf<float4>& image, double& gather_ms, Strip strip, Rows rows)
{
    const int N = (int)m->ctx.size();
    rt_ctx* root = m->ctx[0];
    const int W = m->width, H = m->height;
    RT_HIP(m, hipSetDevice(root->device));
    int max_rows = 0;
    for (rt_ctx* c : m->ctx) max_rows = std::max(max_rows, rows(c));
    RT_HIP(m, image.ensure((size_t)W * H));
    RT_HIP(m, m->d_staging.ensure((size_t)W * max_rows * (size_t)std::max(1, N - 1)));
    RT_HIP(m, hipStreamSynchronize(root->stream));           // (the staging area is allocated and idle: the sources may write)
    const double tg0 = now_ms();
    // every strip travels on ITS source context's stream — N - 1 independent transfers, each over its own xGMI link on a fully connected
    // node, in flight together — and the first device's stream waits for the N - 1 arrival events before it scatters the rows
    for (int i = 1; i < N; ++i) {
        rt_ctx* c = m->ctx[i];
        const size_t pixels = (size_t)W * rows(c);
        if (pixels == 0) continue;
        float4* dst = m->d_staging.p + (size_t)(i - 1) * W * max_rows;
        RT_HIP(m, hipSetDevice(c->device));
        if (c->device == root->device && !root->opt_peer_copies) RT_HIP(m, hipMemcpyAsync(dst, strip(c), pixels * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
        else RT_HIP(m, hipMemcpyPeerAsync(dst, root->device, strip(c), c->device, pixels * sizeof(float4), c->stream));
        RT_HIP(m, hipEventRecord(m->ev_strip[i], c->stream));
    }
    RT_HIP(m, hipSetDevice(root->device));
    for (int i = 1; i < N; ++i)
        if (rows(m->ctx[i]) != 0) RT_HIP(m, hipStreamWaitEvent(root->stream, m->ev_strip[i], 0));
    for (int i = 0; i < N; ++i) {
        rt_ctx* c = m->ctx[i];
        if (rows(c) == 0) continue;
        const float4* src = i == 0 ? strip(c) : m->d_staging.p + (size_t)(i - 1) * W * max_rows;
        const int bands = (rows(c) + 7) / 8;
        hipLaunchKernelGGL(k_scatter_bands, dim3(std::max(1, std::min(64, (W * 8 + 255) / 256)), bands), dim3(256), 0, root->stream, src, image.p, W, H, i, N);
    }
    RT_HIP(m, hipGetLastError());
    RT_HIP(m, hipStreamSynchronize(root->stream));
    gather_ms = now_ms() - tg0;                 // host wall time from the first copy's submission to the assembled image (the copies run on N - 1 streams)
    return 0;
}

// rt_multi_render (params null) and rt_multi_render_params (frame f with params[f] on every context)
int multi_render(rt_multi* m, int first_frame, int n_frames, const rt_params* params)
{
    if (!m->have_params) return fail(m, -2, "rt_multi_set_params has not been called");
    { int r = multi_share_scene(m, [&](rt_ctx* root) { return launch_frames(root, first_frame, 0, Variant::Fast); }); if (r) return r; }
    // every device renders its bands for all frames, concurrently
    { int r = on_every_context(m, params ? "rt_render_params" : "rt_render", [&](int i) {
          return params ? rt_render_params(m->ctx[i], first_frame, n_frames, params) : rt_render(m->ctx[i], first_frame, n_frames); });
      if (r) return r; }
    // ---- the one gather: strips -> first device, rows to their places
    if ((size_t)m->width * m->height == 0) return 0;
    return gather_strips(m, m->d_image, m->lastGatherMs, [](rt_ctx* c) { return c->d_accum.p; }, [](rt_ctx* c) { return c->target.rows; });
}

// Every query entry of the handle (`what`; host_what: the context entry behind it): one contiguous slice of the batch per context,
// traced concurrently, each slice's results written in place.  A sampled family's items keep the stream indices they have in the
// whole batch.
int multi_query(rt_multi* m, QueryDescribe describe, const char* what, const char* host_what, bool need_params, const rt_ray* in, int n, const void* params, void* out)
{
    if (!m) return -1;
    if (need_params && !m->have_params) return fail(m, -2, "%s: rt_multi_set_params has not been called", what);
    QueryCall q;
    if (describe(m->ctx[0], what, in, n, params, out, q)) return fail(m, -2, "%s", rt_last_error(m->ctx[0]));
    if (n == 0) return 0;
    { int r = multi_share_scene(m, [&](rt_ctx* root) { RT_SETTLE(root); return query_prepare(root, 0.f); }); if (r) return r; }
    const int N = (int)m->ctx.size();
    const int per = (n + N - 1) / N;
    return on_every_context(m, host_what, [&](int i) {
        const int first = std::min(n, i * per), cnt = std::min(n, first + per) - first;
        rt_gather_params pi = q.p;              // (ray queries take none; the others' params go through as they came)
        pi.firstIndex = q.p.firstIndex + (uint32_t)first;
        return query_entry(m->ctx[i], describe, host_what, false, in + first, cnt, q.sampled() ? &pi : params, static_cast<char*>(out) + q.out_bytes * (size_t)first);
    });
}

// What the denoiser and the temporal step share behind the handle: every context settled and holding current strips of the image
// (if `image`) and of both feature planes with a frame in them, then those strips gathered to the first device
int multi_gather_inputs(rt_multi* m, const char* what, bool image)
{
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        rt_ctx* c = m->ctx[i];
        { const int r = settle(c); if (r) return fail(m, r, "context %zu: %s", i, rt_last_error(c)); }
        StripLayout L;
        if (strip_layout(c, L)) return fail(m, -2, "context %zu: %s", i, rt_last_error(c));
        L.w = m->width; L.h = m->height;        // (the image the handle assembles, whatever a context was told directly)
        const bool image_current = L == c->target;
        if (L.rows != 0 && (!aov_current(c, L) || c->aov_info.framesAccumulated == 0)) return fail(m, -2, "%s: no feature frame accumulated on context %zu (call rt_multi_render_aov first)", what, i);
        if (image && !image_current) return fail(m, -2, "%s: nothing rendered yet on context %zu", what, i);
    }
    double gather_ms = 0;
    if (image) { int r = gather_strips(m, m->d_image, gather_ms, [](rt_ctx* c) { return c->d_accum.p; }, [](rt_ctx* c) { return c->target.rows; }); if (r) return r; }
    { int r = gather_strips(m, m->d_dn_albedo, gather_ms, [](rt_ctx* c) { return c->d_aov[RT_AOV_ALBEDO].p; }, [](rt_ctx* c) { return c->aov.rows; }); if (r) return r; }
    { int r = gather_strips(m, m->d_dn_guide, gather_ms, [](rt_ctx* c) { return c->d_aov[RT_AOV_NORMAL_DEPTH].p; }, [](rt_ctx* c) { return c->aov.rows; }); if (r) return r; }
    return 0;
}

// The handle's half of the filters' host path (begin_filter / filter_inputs of a context, above): T first, if that is the source, then
// the gather to the first device, whose stream and events run the filter
int begin_filter(rt_multi* m, const char* what)
{
    return m->have_params ? 0 : fail(m, -2, "%s: rt_multi_set_params has not been called", what);
}
int filter_inputs(rt_multi* m, const FilterCall& k, bool from_T, FilterInputs& I)
{
    if (from_T) { int r = temporal_source(m, m->tp, m->width, m->height, k, "rt_multi_temporal", "handle's"); if (r) return r; }
    { int r = multi_gather_inputs(m, k.what, !from_T); if (r) return r; }
    rt_ctx* root = m->ctx[0];
    RT_HIP(m, hipSetDevice(root->device));
    I.C = from_T ? m->tp.t[m->tp.cur].p : m->d_image.p; I.A = m->d_dn_albedo.p; I.G = m->d_dn_guide.p;
    I.W = m->width; I.H = m->height; I.cam = &root->params;
    I.stream = root->stream; I.ev0 = root->ev_dn0; I.ev1 = root->ev_dn1;
    return 0;
}
} // namespace

extern "C" {

int rt_multi_trace_rays(rt_multi* m, const rt_ray* rays, int n, rt_hit* hits) { return multi_query(m, trace_rays_call, "rt_multi_trace_rays", "rt_trace_rays", false, rays, n, nullptr, hits); }
int rt_multi_occluded(rt_multi* m, const rt_ray* rays, int n, uint8_t* occluded) { return multi_query(m, occluded_call, "rt_multi_occluded", "rt_occluded", false, rays, n, nullptr, occluded); }
int rt_multi_trace_radiance(rt_multi* m, const rt_ray* rays, int n, const rt_radiance_params* params, float* rgba) { return multi_query(m, radiance_call, "rt_multi_trace_radiance", "rt_trace_radiance", true, rays, n, params, rgba); }
int rt_multi_gather(rt_multi* m, const rt_ray* points, int n, const rt_gather_params* params, float* out) { return multi_query(m, gather_call, "rt_multi_gather", "rt_gather", true, points, n, params, out); }
int rt_multi_visibility(rt_multi* m, const rt_ray* points, int n, const rt_visibility_params* params, float* out) { return multi_query(m, visibility_call, "rt_multi_visibility", "rt_visibility", false, points, n, params, out); }
int rt_multi_trace_hits(rt_multi* m, const rt_ray* rays, int n, const rt_hits_params* params, rt_multihit* out) { return multi_query(m, hits_call, "rt_multi_trace_hits", "rt_trace_hits", false, rays, n, params, out); }
int rt_multi_closest_points(rt_multi* m, const rt_ray* points, int n, rt_closest* out) { return multi_query(m, closest_call, "rt_multi_closest_points", "rt_closest_points", false, points, n, nullptr, out); }

// Feature buffers behind the handle: the scene is shared as for a render, every context renders the feature frames of its bands
int rt_multi_render_aov(rt_multi* m, int first_frame, int n_frames)
{
    if (!m) return -1;
    if (!m->have_params) return fail(m, -2, "rt_multi_set_params has not been called");
    if (n_frames < 0) return fail(m, -2, "rt_multi_render_aov: n_frames < 0");
    if (n_frames == 0) return 0;
    { int r = multi_share_scene(m, [&](rt_ctx* root) { RT_SETTLE(root); return query_prepare(root, 0.f); }); if (r) return r; }
    return on_every_context(m, "rt_render_aov", [&](int i) { return rt_render_aov(m->ctx[i], first_frame, n_frames); });
}

int rt_multi_read_aov(rt_multi* m, int which, float* rgba, size_t n_floats)
{
    if (!m) return -1;
    if (which < 0 || which >= RT_AOV_COUNT) return fail(m, -2, "unknown feature plane %d", which);
    if (!m->have_params) return fail(m, -2, "rt_multi_set_params has not been called");
    if (!rgba) return fail(m, -2, "null destination");
    return read_image(m, (size_t)m->width * m->height * 4, rgba, n_floats, [&](const float4*& src) {
        // (a context that has rendered no feature frame yet holds zeroed planes of its strip)
        { int r = for_each_ctx(m, "feature planes", [&](rt_ctx* c) { RT_SETTLE(c); RT_HIP(c, hipSetDevice(c->device)); return ensure_aov(c); }); if (r) return r; }
        double gather_ms = 0;
        { int r = gather_strips(m, m->d_aov_image, gather_ms, [&](rt_ctx* c) { return c->d_aov[which].p; }, [](rt_ctx* c) { return c->aov.rows; }); if (r) return r; }
        src = m->d_aov_image.p;
        return 0;
    });
}

int rt_multi_reset_aov(rt_multi* m) { return m ? for_each_ctx(m, "rt_reset_aov", [&](rt_ctx* c) { return rt_reset_aov(c); }) : -1; }

// The image filters behind the handle: image and both feature planes gathered to the first device, the context's filter there, the
// planes and the temporal state on the handle.  Its reads take the first context's stream (every producer has waited before it returned)
int rt_multi_denoise(rt_multi* m, const rt_denoise_params* params) { return denoise_call(m, { "rt_multi_denoise", nullptr }, false, params); }
int rt_multi_temporal(rt_multi* m, const rt_temporal_params* params) { return temporal_call(m, { "rt_multi_temporal", nullptr }, params); }
int rt_multi_denoise_temporal(rt_multi* m, const rt_denoise_params* params)
{
    return denoise_call(m, { "rt_multi_denoise_temporal", nullptr }, true, params);
}
int rt_multi_denoise_variance(rt_multi* m, const rt_vdenoise_params* params)
{
    return denoise_variance_call(m, { "rt_multi_denoise_variance", nullptr, "source 1, and " }, params);
}

int rt_multi_reset_temporal(rt_multi* m)
{
    if (!m) return -1;
    m->tp.reset();
    return 0;
}

int rt_multi_read_temporal(rt_multi* m, float* rgba, size_t n)
{
    return m ? read_filter_plane(m, m->ctx[0], m->tp, "rt_multi_temporal", m->tp.t[m->tp.cur].p, 4, rgba, n, false) : -1;
}
int rt_multi_read_temporal_history(rt_multi* m, float* hist, size_t n)
{
    return m ? read_filter_plane(m, m->ctx[0], m->tp, "rt_multi_temporal", m->tp.n[m->tp.cur].p, 1, hist, n, false) : -1;
}
int rt_multi_read_temporal_display(rt_multi* m, uint32_t* rgba8, size_t n_pixels)
{
    return m ? read_filter_display(m, m->ctx[0], m->tp, "rt_multi_temporal", m->tp.t[m->tp.cur].p, m->d_display, rgba8, n_pixels) : -1;
}
int rt_multi_read_variance(rt_multi* m, float* var, size_t n)
{
    return m ? read_filter_plane(m, m->ctx[0], m->vd, "rt_multi_denoise_variance", m->vd.var.p, 1, var, n, false) : -1;
}
// (whichever filter filled the denoised plane, the message names rt_multi_denoise)
int rt_multi_read_denoised(rt_multi* m, float* rgba, size_t n)
{
    return m ? read_filter_plane(m, m->ctx[0], m->dn, "rt_multi_denoise", m->dn.out.p, 4, rgba, n, false) : -1;
}
int rt_multi_read_denoised_display(rt_multi* m, uint32_t* rgba8, size_t n_pixels)
{
    return m ? read_filter_display(m, m->ctx[0], m->dn, "rt_multi_denoise", m->dn.out.p, m->d_display, rgba8, n_pixels) : -1;
}

int rt_multi_render(rt_multi* m, int first_frame, int n_frames)
{
    if (!m) return -1;
    return multi_render(m, first_frame, n_frames, nullptr);
}

int rt_multi_render_params(rt_multi* m, int first_frame, int n_frames, const rt_params* params)
{
    if (!m) return -1;
    if (n_frames < 0) return fail(m, -2, "n_frames < 0");
    if (n_frames == 0) return 0;
    if (!params) return fail(m, -2, "null params");
    if (const int f = other_settings(params, n_frames)) return fail(m, -2, "rt_multi_render_params: entry %d differs from entry 0 outside the camera fields", f);
    if (!m->have_params || !same_settings(m->ctx[0]->params, params[0])) { const int r = rt_multi_set_params(m, &params[0]); if (r) return r; }
    return multi_render(m, first_frame, n_frames, params);
}

// The display step for the assembled image (rt_read_display's twin): linear -> sRGB8 on the first device.
int rt_multi_read_display(rt_multi* m, uint32_t* rgba8, size_t n_pixels)
{
    if (!m) return -1;
    if (!rgba8 && n_pixels) return fail(m, -2, "null destination");
    return read_srgb8(m, m->ctx[0], m->d_image.p, (size_t)m->width * m->height, m->d_display, rgba8, n_pixels);
}

// Restore a saved accumulation state (rt_write_accum's twin): the whole image goes in, every context takes the rows of its bands.
int rt_multi_write_accum(rt_multi* m, const float* rgba, size_t n_floats, int frames_rendered)
{
    if (!m) return -1;
    if (!m->have_params) return fail(m, -2, "rt_multi_set_params has not been called");
    if (!rgba && n_floats) return fail(m, -2, "null source");
    const int W = m->width, H = m->height, N = (int)m->ctx.size();
    if (n_floats != (size_t)W * H * 4) return fail(m, -2, "expected %zu floats (height*width*4), got %zu", (size_t)W * H * 4, n_floats);
    std::vector<float> strip;
    for (int i = 0; i < N; ++i) {
        strip.clear();
        for (int y0 = i * 8; y0 < H; y0 += N * 8) {
            const int rows = std::min(8, H - y0);
            strip.insert(strip.end(), rgba + (size_t)y0 * W * 4, rgba + (size_t)(y0 + rows) * W * 4);
        }
        const int r = rt_write_accum(m->ctx[i], strip.data(), strip.size(), frames_rendered);
        if (r) return fail(m, r, "rt_write_accum on context %d: %s", i, rt_last_error(m->ctx[i]));
    }
    // the assembled image follows, so that rt_multi_read_accum / rt_multi_read_display show the restored state before the next render
    rt_ctx* root = m->ctx[0];
    RT_HIP(m, hipSetDevice(root->device));
    RT_HIP(m, m->d_image.ensure((size_t)W * H));
    if (n_floats) RT_HIP(m, hipMemcpy(m->d_image.p, rgba, n_floats * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int rt_multi_read_accum(rt_multi* m, float* rgba, size_t n_floats)
{
    if (!m) return -1;
    if (!rgba && n_floats) return fail(m, -2, "null destination");
    return read_image(m, (size_t)m->width * m->height * 4, rgba, n_floats, [&](const float4*& src) {
        src = m->d_image.p;
        return src ? 0 : fail(m, -2, "nothing rendered yet");
    });
}

int rt_multi_get_stats(rt_multi* m, rt_stats* out, double* gather_ms)
{
    if (!m) return -1;
    if (!out) return fail(m, -2, "null stats");
    rt_stats sum = m->ctx[0]->stats;
    for (size_t i = 1; i < m->ctx.size(); ++i) {
        const rt_stats& s = m->ctx[i]->stats;
        const double last_ms = std::max(sum.lastKernelMs, s.lastKernelMs);      // (kernel times: the slowest context's)
        add_launch_stats(sum, s);
        sum.lastKernelMs = last_ms; sum.totalKernelMs = std::max(sum.totalKernelMs, s.totalKernelMs);
    }
    *out = sum;
    if (gather_ms) *gather_ms = m->lastGatherMs;
    return 0;
}

int rt_multi_get_info(rt_multi* m, rt_multi_info* out)
{
    if (!m) return -1;
    if (!out) return fail(m, -2, "null info");
    std::memset(out, 0, sizeof *out);
    out->numContexts = (int32_t)m->ctx.size();
    for (rt_ctx* c : m->ctx) out->bvhBuilds += c->stats.bvhBuilds;
    out->lastSetupMs = m->lastSetupMs; out->lastGatherMs = m->lastGatherMs;
    for (size_t i = 0; i < m->ctx.size() && i < 16; ++i) { out->device[i] = m->ctx[i]->device; out->peerAccess[i] = m->peer[i]; }
    return 0;
}

} // extern "C"
