// rt_render.hip — frames: the launch planner (plan_launch .. launch_frames), tile order, camera-ray lists, the camera table, the
// submission queue, the accumulation target and its reads, the feature buffers, and the row scatter of rt_multi's gather.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <type_traits>

#include "rt_ctx.hpp"
#include "rt_kernels.hpp"
#include "rt_stream.hpp"
namespace rtk {
const void* stream_kernel(bool counting, bool philox, bool compact, bool triangles);        // rt_stream_kernels.hip
const void* cam_stream_kernel(bool philox, bool compact, bool triangles);
}
#include "rt_primary.hpp"
#include "rt_aov.hpp"

using namespace rth;

int rth::ensure_targets(rt_ctx* c)
{
    StripLayout L;
    { int r = strip_layout(c, L); if (r) return r; }
    if (L == c->target) return 0;           // (a context that never rendered holds the layout of an empty image)
    { int r = create_planes(c, L, { &c->d_frame, &c->d_accum }); if (r) return r; }
    c->target = L; c->tile_order_valid = false;
    c->stats.numRenderedFrames = 0; c->stats.totalKernelMs = 0;
    return 0;
}

// The camera fields of rt_params (viewParams, camLocalToWorld, worldSpaceCameraPos: what UpdateCameraParams sets, plus _WorldSpaceCameraPos)
// are one contiguous range; every other field is a setting.
constexpr size_t kCamBegin = offsetof(rt_params, viewParams), kCamEnd = offsetof(rt_params, worldSpaceLightPos0);
static_assert(offsetof(rt_params, camLocalToWorld) == kCamBegin + 12 && offsetof(rt_params, worldSpaceCameraPos) == kCamBegin + 76
              && kCamEnd == kCamBegin + 88, "the camera fields of rt_params are contiguous");
bool rth::same_settings(const rt_params& a, const rt_params& b)
{
    return std::memcmp(&a, &b, kCamBegin) == 0 && std::memcmp((const char*)&a + kCamEnd, (const char*)&b + kCamEnd, sizeof(rt_params) - kCamEnd) == 0;
}
// the first entry of params[0 .. n - 1] whose settings differ from entry 0's, 0 if none does (rt_render_params, rt_multi_render_params)
int rth::other_settings(const rt_params* params, int n)
{
    for (int f = 1; f < n; ++f) if (!same_settings(params[f], params[0])) return f;
    return 0;
}

// the per-launch figures of rt_stats summed over the launches of one call
void rth::add_launch_stats(rt_stats& sum, const rt_stats& s)
{
    sum.rays += s.rays; sum.sphereTests += s.sphereTests; sum.nodeVisits += s.nodeVisits; sum.triTests += s.triTests; sum.hits += s.hits;
    for (int k = 0; k < 5; ++k) { sum.phaseLanes[k] += s.phaseLanes[k]; sum.phaseExecs[k] += s.phaseExecs[k]; }
    for (int k = 0; k < rtk::kNumRegions; ++k) sum.regionExecs[k] += s.regionExecs[k];
    sum.lastKernelMs += s.lastKernelMs;
}

namespace {

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

// p (same settings as c->params) becomes the context's params, as rt_set_params(p) would make it
void use_camera(rt_ctx* c, const rt_params& p)
{
    if (std::memcmp(&c->params, &p, sizeof p) != 0) c->tile_order_stale = true;
    c->params = p;
}

void set_launch_stats(rt_stats& st, const rt_stats& sum)
{
    st.rays = sum.rays; st.sphereTests = sum.sphereTests; st.nodeVisits = sum.nodeVisits; st.triTests = sum.triTests; st.hits = sum.hits;
    for (int k = 0; k < 5; ++k) { st.phaseLanes[k] = sum.phaseLanes[k]; st.phaseExecs[k] = sum.phaseExecs[k]; }
    for (int k = 0; k < rtk::kNumRegions; ++k) st.regionExecs[k] = sum.regionExecs[k];
    st.lastKernelMs = sum.lastKernelMs;
}

// What a launch_frames_k call launches, and with which arguments
struct LaunchPlan {
    rtk::DeviceScene S{}; rtk::FrameArgs F{}; rtk::StreamArgs A{};
    const void* fn = nullptr; size_t lds = 0;
    int grid = 1, batch = 1, ntiles = 0, sample_lanes_log2 = 0;
    bool philox = false, stream = false, tile_kernel = false, stream_sync = false, cam_table = false, record_costs = false;
};

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
    const void* fn = P.fn = stream ? (cams ? rtk::cam_stream_kernel(philox, compact, c->n_nodes > 0)
                                           : rtk::stream_kernel(counting, philox, compact, c->n_nodes > 0))     // instantiated in rt_stream_kernels.hip
                                   : trace_kernel(counting, var == Variant::Flat, compact, c->n_nodes == 0);    // ... in rt_api.hip
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
    A.shade_threshold = c->opt_shade_threshold;         // (1..64: rt_set_option)
    A.total_pixels = (unsigned int)P.ntiles * 64u;
    A.tile_sync = stream_sync ? 1 : 0;
    A.sample_lanes_log2 = P.sample_lanes_log2;
    A.tiles_per_fetch = std::max(1, std::min(rtk::kGroupMax, c->opt_tiles_per_fetch));      // (the option takes 1..64, a group holds kGroupMax)
    A.guide_div = 1;
    A.node_min = c->opt_node_min;                       // (1..64: rt_set_option)
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
        { int r = sort_tiles_by_cost(c, (uint32_t)P.ntiles); if (r) return r; }
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

} // namespace

// Kernel choice "auto" (option kernel = -1, the default): k_trace and k_stream (resumable traversal, stragglers deferred)
// produce the same bits, and which one is faster depends on the scene (measured: k_stream +8 % on the 100k-triangle
// workload, -5 % on the 1M-triangle one, -13 % on spheres only).  So the first frames after a scene / camera change are
// used as the measurement: one frame records the tile costs, one is timed with k_trace, one with k_stream (all three are
// ordinary frames of the render — nothing is traced twice); the faster kernel takes the rest.
int rth::launch_frames(rt_ctx* c, int first_frame, int n_frames, Variant var, const rt_params* cams)
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

namespace {

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

} // namespace

// Every entry point but rt_submit_frame starts here: the queue is empty and the worker idle before anything else touches the context
// (a context has one caller thread; the worker is the library's own).  Returns the first error a queued launch met, once.
int rth::settle(rt_ctx* c)
{
    if (!c->q_started) return 0;
    std::unique_lock<std::mutex> lk(c->q_mu);
    c->q_idle.wait(lk, [&] { return c->q_frames.empty() && !c->q_busy; });
    const int r = c->q_rc;
    if (r) { c->err = "queued frame: " + c->q_err; c->q_rc = 0; }
    return r;
}

// ---- feature buffers (rt_render_aov, csrc/rt_aov.hpp) -----------------------------------------------------------------------------
// The two planes of the context's strip, zeroed when they are created and whenever the strip's layout changes (ensure_targets' rule for
// the accumulation target, kept apart from it: a feature frame must not touch the image path's state)
bool rth::aov_current(const rt_ctx* c, const StripLayout& L) { return c->d_aov[0].p && L == c->aov; }
int rth::ensure_aov(rt_ctx* c)
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

namespace {

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
    const void* fn = c->opt_compact_nodes != 0 ? (const void*)rtk::k_aov<true> : (const void*)rtk::k_aov<false>;    // (the node form plan_launch picks)
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

void rth::scatter_bands(hipStream_t stream, const float4* strip, float4* image, int W, int H, int rank, int N, int bands)
{
    hipLaunchKernelGGL(k_scatter_bands, dim3(std::max(1, std::min(64, (W * 8 + 255) / 256)), bands), dim3(256), 0, stream, strip, image, W, H, rank, N);
}

extern "C" {

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

} // extern "C"
