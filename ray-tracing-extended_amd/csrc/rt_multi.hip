// rt_multi.hip — several devices behind one handle (struct rt_multi, rt_ctx.hpp): every rt_multi_* entry of include/rt.h.
// Host code only: the handle drives its contexts through their own entries and the shared steps of rt_ctx.hpp; no kernel lives here.
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rt_ctx.hpp"

using namespace rth;

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
        scatter_bands(root->stream, src, image.p, W, H, i, N, (rows(c) + 7) / 8);
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
} // namespace

// The handle's half of the filters' host path (begin_filter / filter_inputs of a context, rt_filters.hip): T first, if that is the
// source, then the gather to the first device, whose stream and events run the filter
int rth::begin_filter(rt_multi* m, const char* what)
{
    return m->have_params ? 0 : fail(m, -2, "%s: rt_multi_set_params has not been called", what);
}
int rth::filter_inputs(rt_multi* m, const FilterCall& k, bool from_T, FilterInputs& I)
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
