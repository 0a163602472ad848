// rt_queries.hip — the one path of the six query families: ray queries and sphere casts, radiance queries, gather queries, visibility
// gathers, closest-point / K-nearest / box and capsule overlap queries and multi-hit ray queries; their entries and info getters.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "rt_ctx.hpp"
#include "rt_query.hpp"
#include "rt_radiance.hpp"
#include "rt_gather.hpp"
#include "rt_visibility.hpp"
#include "rt_multihit.hpp"
#include "rt_sweep.hpp"
#include "rt_sweep_all.hpp"
#include "rt_listed.hpp"            // NearestArgs and rt_closest.hpp's walk; k_closest, k_nearest, k_overlap and k_capsule themselves: rt_api.hip closest_kernel

using namespace rth;

// One launch: `n` items from `in`, results to `out`, item 0 with stream index first_index
struct rth::QuerySlice { const rtk::DeviceScene* S; const float4* in; void* out; int n; uint32_t first_index; int grid; LaneStack st; };

namespace {

// ---- ray queries (rt_trace_rays / rt_occluded, csrc/rt_query.hpp) ---------------------------------------------------------------
// Largest finite |origin coordinate| over the rays a query traces (tMax > 0)
// both_ends (capsule overlap queries): an input is a segment, and its other endpoint origin + direction counts as well
float query_origin_bound(const rt_ray* rays, int n, bool both_ends)
{
    float m = 0.f;
    for (int i = 0; i < n; ++i) {
        if (!(rays[i].tMax > 0.0f)) continue;
        for (int a = 0; a < 3; ++a) { const float v = std::fabs(rays[i].origin[a]); if (v > m && v <= 3.4028235e38f) m = v; }
        if (!both_ends) continue;
        for (int a = 0; a < 3; ++a) { const float v = std::fabs(rays[i].origin[a] + rays[i].direction[a]); if (v > m && v <= 3.4028235e38f) m = v; }
    }
    return m;
}

// p lies in memory of the context's device (hipMalloc'ed or managed)
bool on_ctx_device(const rt_ctx* c, const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.isManaged) && a.device == c->device;
}

} // namespace

// Settle, then make the scene current for rays whose origins reach |coordinate| G (host entries; the device entries measure G on the
// device between the two steps, query_prepare_device)
int rth::query_prepare(rt_ctx* c, float G)
{
    RT_HIP(c, hipSetDevice(c->device));
    { int r = prepare_scene(c); if (r) return r; }
    return cover_origins(c, G);
}

namespace {

// ---- the one path of the six query families ----------------------------------------------------------------------------------------
// Ray queries (rt_trace_rays / rt_occluded, csrc/rt_query.hpp), radiance queries (rt_trace_radiance, csrc/rt_radiance.hpp), gather
// queries (rt_gather, csrc/rt_gather.hpp), visibility gathers (rt_visibility, csrc/rt_visibility.hpp), closest-point queries
// (rt_closest_points, csrc/rt_closest.hpp) and multi-hit ray queries (rt_trace_hits, csrc/rt_multihit.hpp) all take n rt_ray (2 float4 each) and write a fixed number of bytes per item.  A family supplies a description of the call (QueryCall, rt_ctx.hpp, built by its *_call once
// the arguments are known to be good) and a function that fills its kernel's Args for one launch; everything between the exported
// entry and hipLaunchKernel is below, once.

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

// A kernel's instantiation for the node form the renderer's kernels traverse (rt_render.hip plan_launch): k<..., true> for compact nodes
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
    { int r = query_prepare(c, query_origin_bound(in, n, q.both_ends)); if (r) return r; }
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
    { int r = cover_origins_device(c, static_cast<const float4*>(in), n, q.both_ends); if (r) return r; }
    if (q.begin) { int r = q.begin(c); if (r) return r; }
    { int r = launch_slices(c, q, static_cast<const float4*>(in), out, n, q.p.firstIndex); if (r) return r; }
    if (q.timed()) c->query_info[q.family].calls++;
    return 0;
}

// ---- the six descriptions --------------------------------------------------------------------------------------------------------
// A *_call checks the arguments of a call to `what` and describes it; all have the signature of QueryDescribe (ray queries and
// closest-point queries take no params; multi-hit queries take their own, which are not the sampled families').  The checks come in one order: params set (where the family needs them), n and the pointers, the defaults of
// params == NULL, samples, mode, reserved words.
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

hipError_t launch_radiance(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::RadianceArgs A{};
    fill_sampled(c, q, s, A);
    A.p = c->params;
    return launch_slice(c, pick_nodes(c, rtk::k_radiance<true>, rtk::k_radiance<false>), s, A);
}

hipError_t launch_gather(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::GatherArgs A{};
    fill_sampled(c, q, s, A);
    A.p = c->params;
    return launch_slice(c, q.p.mode == RT_GATHER_SH9 ? pick_nodes(c, rtk::k_gather<RT_GATHER_SH9, true>, rtk::k_gather<RT_GATHER_SH9, false>)
                                                     : pick_nodes(c, rtk::k_gather<RT_GATHER_COSINE, true>, rtk::k_gather<RT_GATHER_COSINE, false>), s, A);
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
hipError_t launch_closest(rt_ctx* c, const QueryCall&, const QuerySlice& s)
{
    // K-nearest queries: the same points and launch shape, K records each (csrc/rt_nearest.hpp); k_closest takes the Args' ClosestArgs part
    // box overlap queries ("closest_box" = 1): each input is a box, whatever K and all are (csrc/rt_overlap.hpp)
    // capsule overlap queries ("closest_capsule" = 1): each input is a segment, whatever K and all are (csrc/rt_capsule.hpp)
    const bool nearest = c->opt_closest_k != 1 || c->opt_closest_all, box = c->opt_closest_box != 0;
    rtk::NearestArgs A{};
    fill_head(c, s, A);
    A.out = static_cast<float4*>(s.out);
    A.counters = c->opt_closest_count ? c->d_closest_counts.p : nullptr;
    A.k = c->opt_closest_k; A.count_all = c->opt_closest_all;
    return launch_slice(c, closest_kernel(c->opt_compact_nodes != 0, c->opt_closest_count != 0, nearest, box, c->opt_closest_capsule != 0), s, A);     // (instantiated in rt_api.hip)
}

hipError_t launch_hits(rt_ctx* c, const QueryCall& q, const QuerySlice& s)
{
    rtk::MultihitArgs A{};
    fill_head(c, s, A);
    A.max_hits = q.h.maxHits; A.count_all = q.h.countAll;
    A.out = static_cast<float4*>(s.out);
    c->hits_last = q.h;
    // sphere-cast-all ("hits_sweep" = 1): the same rays, records and launch shape; the params' mode is validated and not read (csrc/rt_sweep_all.hpp)
    if (c->opt_hits_sweep) return launch_slice(c, pick_nodes(c, rtk::k_sweep_all<true>, rtk::k_sweep_all<false>), s, A);
    if (q.h.mode == RT_HITS_BOTH) return launch_slice(c, pick_nodes(c, rtk::k_multihit<true, true>, rtk::k_multihit<false, true>), s, A);
    return launch_slice(c, pick_nodes(c, rtk::k_multihit<true, false>, rtk::k_multihit<false, false>), s, A);
}

} // namespace

// n rt_hit (4 float4 each) / n occlusion bytes
int rth::trace_rays_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* hits, QueryCall& q)
{
    q = QueryCall{ kRays, what, "rays", "hits", kQuerySlice, sizeof(rt_hit), true, nullptr, launch_rays<false> };
    return query_pointers(c, q, rays, n, hits);
}
int rth::occluded_call(rt_ctx* c, const char* what, const void* rays, int n, const void*, const void* occluded, QueryCall& q)
{
    q = QueryCall{ kRays, what, "rays", "occluded", kQuerySlice, 1, false, nullptr, launch_rays<true> };
    return query_pointers(c, q, rays, n, occluded);
}

// n float4; params == NULL: the context's numRaysPerPixel samples
int rth::radiance_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* rgba, QueryCall& q)
{
    q = QueryCall{ kRadiance, what, "rays", "rgba", c->opt_radiance_slice, sizeof(float4), true, "rt_trace_radiance", launch_radiance };
    return sampled_arguments(c, q, true, rays, n, params, c->params.numRaysPerPixel, rgba, 1, nullptr, "rt_radiance_params");
}

// n or 9 n float4; params == NULL: the context's numRaysPerPixel samples
int rth::gather_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q)
{
    q = QueryCall{ kGather, what, "points", "out", c->opt_gather_slice, 0, true, "rt_gather", launch_gather };
    { int r = sampled_arguments(c, q, true, points, n, params, c->params.numRaysPerPixel, out, 2, "neither RT_GATHER_COSINE nor RT_GATHER_SH9", "rt_gather_params"); if (r) return r; }
    q.out_bytes = sizeof(float4) * (q.p.mode == RT_GATHER_SH9 ? 9 : 1);
    return 0;
}

// n or 3 n float4; params == NULL: RT_VISIBILITY_DEFAULT_SAMPLES samples.  No rt_params are needed: the kernel reads intersectMode
// alone, as the ray queries do
int rth::visibility_call(rt_ctx* c, const char* what, const void* points, int n, const void* params, const void* out, QueryCall& q)
{
    q = QueryCall{ kVisibility, what, "points", "out", c->opt_visibility_slice, 0, true, "rt_visibility", launch_visibility };
    { int r = sampled_arguments(c, q, false, points, n, params, RT_VISIBILITY_DEFAULT_SAMPLES, out, 3, "none of RT_VIS_COSINE, RT_VIS_SH9, RT_VIS_DISTANCE", "rt_visibility_params"); if (r) return r; }
    q.out_bytes = sizeof(float4) * (q.p.mode == RT_VIS_SH9 ? 3 : 1);
    return 0;
}

// n * K rt_closest (4 float4 each), K = option "closest_k"; no params of either kind.  The points per launch are min("closest_slice",
// 4194304 / K): the staged results never exceed the 256 MiB of K = 1
int rth::closest_call(rt_ctx* c, const char* what, const void* points, int n, const void*, const void* out, QueryCall& q)
{
    const int K = c->opt_closest_k;
    q = QueryCall{ kClosest, what, "points", "out", std::min(c->opt_closest_slice, kQuerySlice / K), sizeof(rt_closest) * (size_t)K, true, nullptr, launch_closest };
    q.begin = begin_closest;
    q.both_ends = c->opt_closest_capsule != 0;          // a segment's other endpoint needs the box padding too
    return query_pointers(c, q, points, n, out);
}

// n * K rt_multihit (4 float4 each); params == NULL: RT_HITS_DEFAULT_MAX records per ray, front faces, hitCount capped at K.  No
// rt_params are needed: the kernel reads intersectMode alone, as the ray queries do
int rth::hits_call(rt_ctx* c, const char* what, const void* rays, int n, const void* params, const void* out, QueryCall& q)
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
int rth::query_entry(rt_ctx* c, QueryDescribe describe, const char* what, bool device, const void* in, int n, const void* params, void* out)
{
    if (!c) return -1;
    RT_SETTLE(c);
    QueryCall q;
    { int r = describe(c, what, in, n, params, out, q); if (r) return r; }
    return device ? query_device(c, q, in, n, out) : query_host(c, q, static_cast<const rt_ray*>(in), n, out);
}

extern "C" {

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
// (the three info records are one layout, checked where the path begins)
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

} // extern "C"
