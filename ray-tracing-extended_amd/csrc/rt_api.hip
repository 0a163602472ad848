// rt_api.hip — C-ABI of include/rt.h on top of the HIP kernels (gfx950 only, no CPU fallback).
//
// Host-side counterpart of RayTracingManager.OnRenderImage / InitFrame (RayTracingManager.cs:49-124) below
// the Material.Set* / Graphics.Blit boundary: owns the device copies of the three structured buffers, the
// accumulation target (resultTexture) and the per-frame target (currentFrame).
//
// This unit: the context's life cycle, uploads, options, rows and bands, scene builds and refits, the on-device geometry pipeline, the
// plane copies and the display step.  The other units of the library and what crosses between them: rt_ctx.hpp.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt_ctx.hpp"
#include "rt_geom.hpp"
#include "rt_bvh_gpu.hpp"
#include "rt_nearest.hpp"
#include "rt_overlap.hpp"
#include "rt_capsule.hpp"           // (with rt_listed.hpp, rt_closest.hpp and rt_query.hpp: trace_kernel .. cover_origins_device below)

using namespace rth;

thread_local std::string rth::g_create_error;

int rth::fail(ErrOwner* owner, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (owner) owner->err = buf; else g_create_error = buf;
    return code;
}

// Largest |coordinate| a camera-ray origin can have: camera position plus the defocus disc (frag :377-378).
float rth::camera_magnitude(const rt_params& p)
{
    float m = 0.f;
    for (int a = 0; a < 3; ++a) m = std::max(m, std::fabs(p.worldSpaceCameraPos[a]));
    float jitter = std::fabs(p.defocusStrength) / std::max(1.0f, (float)p.width);
    float axis = 0.f;
    for (int a = 0; a < 3; ++a)
        axis = std::max(axis, std::fabs(p.camLocalToWorld[4 * a]) + std::fabs(p.camLocalToWorld[4 * a + 1]));
    return m + jitter * axis;
}

namespace {

void pack_material(const rt_material& m, float4* out)
{
    out[0] = f4(m.colour); out[1] = f4(m.emissionColour); out[2] = f4(m.specularColour);
    out[3] = make_float4(m.emissionStrength, m.smoothness, m.specularProbability, u2f((uint32_t)m.flag));
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

// b = s's contents, device to device (clone_scene)
template <class T> int clone_buf(rt_ctx* dst, DevBuf<T>& d, const rt_ctx* src, const DevBuf<T>& s)
{
    RT_HIP(dst, d.ensure(s.used));
    if (!s.used) return 0;
    if (dst->device == src->device && !dst->opt_peer_copies) RT_HIP(dst, hipMemcpyAsync(d.p, s.p, s.used * sizeof(T), hipMemcpyDeviceToDevice, dst->stream));
    else RT_HIP(dst, hipMemcpyPeerAsync(d.p, dst->device, s.p, src->device, s.used * sizeof(T), dst->stream));
    return 0;
}

// the device in whose memory p lies (hipMalloc'ed or managed), -1: host memory (a plain host pointer makes the query fail)
int device_of_ptr(const void* p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.isManaged) ? a.device : -1;
}

} // namespace

// Make the device's scene current for c->params: build what was uploaded, move the meshes, or widen the box padding when a ray origin
// has moved beyond it
int rth::prepare_scene(rt_ctx* c)
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
int rth::cover_origins(rt_ctx* c, float G)
{
    if (!(G > c->bvh.magnitude)) return 0;
    return c->geom_local ? run_geometry_kernels(c, true, G) : repad_boxes(c, std::min(2.0f * G, FLT_MAX));
}

// cover_origins for rays in device memory: the origin bound of the batch is measured on the device — one small kernel and a 4-byte
// read-back (the call's one synchronisation)
int rth::cover_origins_device(rt_ctx* c, const float4* rays, int n, bool both_ends)
{
    RT_HIP(c, c->d_q_bound.ensure(1));
    RT_HIP(c, hipMemsetAsync(c->d_q_bound.p, 0, sizeof(unsigned int), c->stream));
    const int grid = std::max(1, std::min((n + 255) / 256, 4 * std::max(1, c->n_cu)));
    if (both_ends) hipLaunchKernelGGL(rtk::k_query_origin_bound<1>, dim3(grid), dim3(256), 0, c->stream, rays, n, c->d_q_bound.p);     // (a segment's two endpoints)
    else hipLaunchKernelGGL(rtk::k_query_origin_bound<0>, dim3(grid), dim3(256), 0, c->stream, rays, n, c->d_q_bound.p);
    RT_HIP(c, hipGetLastError());
    unsigned int bits = 0;
    RT_HIP(c, hipMemcpyAsync(&bits, c->d_q_bound.p, sizeof bits, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return cover_origins(c, u2f(bits));
}

// The renderer's tile kernel (rt_render.hip plan_launch): the flat validation twin, the spheres-only instantiation compiled for six
// waves per SIMD, or the one for the node form
const void* rth::trace_kernel(bool counting, bool flat, bool compact, bool spheres_only)
{
    if (flat) return (const void*)rtk::k_trace<false, true>;
    if (spheres_only) return counting ? (const void*)rtk::k_trace<true, false, false, 6> : (const void*)rtk::k_trace<false, false, false, 6>;
    if (compact) return counting ? (const void*)rtk::k_trace<true, false, true> : (const void*)rtk::k_trace<false, false, true>;
    return counting ? (const void*)rtk::k_trace<true, false, false> : (const void*)rtk::k_trace<false, false, false>;
}

// k_closest, k_nearest, k_overlap or k_capsule<node form, counting> (rt_queries.hip launch_closest)
template <bool H, bool COUNT> static const void* closest_kernel_of(bool nearest, bool box, bool capsule)
{
    if (capsule) return (const void*)rtk::k_capsule<H, COUNT>;
    return box ? (const void*)rtk::k_overlap<H, COUNT> : nearest ? (const void*)rtk::k_nearest<H, COUNT> : (const void*)rtk::k_closest<H, COUNT>;
}
const void* rth::closest_kernel(bool compact, bool counting, bool nearest, bool box, bool capsule)
{
    if (compact) return counting ? closest_kernel_of<true, true>(nearest, box, capsule) : closest_kernel_of<true, false>(nearest, box, capsule);
    return counting ? closest_kernel_of<false, true>(nearest, box, capsule) : closest_kernel_of<false, false>(nearest, box, capsule);
}

// Give `dst` the scene `src` has built (world-space uploads): every device buffer is copied device to device — over xGMI when the
// contexts sit on different GPUs — and the host-side description of the tree comes along; dst builds nothing and holds no host copy of
// the triangles.  rt_multi uses it so that N contexts cost one BVH build and one host -> device upload per scene change.
int rth::clone_scene(rt_ctx* dst, rt_ctx* src)
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
int rth::strip_layout(rt_ctx* c, StripLayout& L)
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
int rth::create_planes(rt_ctx* c, const StripLayout& L, std::initializer_list<DevBuf<float4>*> planes)
{
    const size_t px = L.pixels();
    for (DevBuf<float4>* b : planes) {
        RT_HIP(c, b->ensure(px));
        if (px) RT_HIP(c, hipMemsetAsync(b->p, 0, px * sizeof(float4), c->stream));
    }
    return 0;
}

// The device scene every kernel reads
int rth::fill_scene(rt_ctx* c, rtk::DeviceScene& S)
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
int rth::tile_stack_cap(const rt_ctx* c)
{
    int cap = std::max(1, c->bvh.maxStack);
    if (c->opt_lds_stack > 0) cap = std::min(cap, c->opt_lds_stack);
    return std::min(cap, 64);
}

// The traversal stack of a launch of such a kernel (k_trace, k_ray_query, k_aov) over `lanes` lanes: tile_stack_cap entries per lane in
// `lds` bytes of LDS per workgroup, and for a deeper tree the global overflow area — one slot per lane of the launch and entry beyond cap,
// so such a tree pays for the launch's width.  refuse_4g_for: the entry point whose launches are as wide as its image and that refuses
// an area above 4 GiB (null: the launch's width is bounded and the area is allocated whatever it takes)
int rth::plan_lane_stack(rt_ctx* c, size_t lanes, LaneStack& st, const char* refuse_4g_for)
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

// Costliest tiles first for the next launches (rt_render.hip finish_launch): counting sort of d_tile_cost into d_tile_order on the
// device, no host round trip
int rth::sort_tiles_by_cost(rt_ctx* c, uint32_t ntiles)
{
    RT_HIP(c, c->d_tile_hist.ensure(rtg::kCostBuckets));
    RT_HIP(c, hipMemsetAsync(c->d_tile_hist.p, 0, rtg::kCostBuckets * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(rtg::k_tile_hist, dim3((ntiles + 255) / 256), dim3(256), 0, c->stream, c->d_tile_cost.p, ntiles, c->d_tile_hist.p);
    hipLaunchKernelGGL(rtg::k_tile_scan, dim3(1), dim3(1024), 0, c->stream, c->d_tile_hist.p);
    hipLaunchKernelGGL(rtg::k_tile_scatter, dim3((ntiles + 255) / 256), dim3(256), 0, c->stream, c->d_tile_cost.p, ntiles,
                       c->d_tile_hist.p, c->d_tile_order.p);
    RT_HIP(c, hipGetLastError());
    return 0;
}

// The end of every read of a plane: n_floats must be the plane's expect_floats (`shape`: what the message calls that product), then one
// copy on the stream of `on` — the context that holds the plane: o itself, or the first context of the handle o — waited for.  What a
// null destination means is the entry point's own rule, checked before.
int rth::copy_plane(ErrOwner* o, const rt_ctx* on, const void* src, size_t expect_floats, const char* shape, void* dst, size_t n_floats, bool to_device)
{
    if (n_floats != expect_floats) return fail(o, -2, "expected %zu floats (%s), got %zu", expect_floats, shape, n_floats);
    if (!n_floats) return 0;
    RT_HIP(o, hipSetDevice(on->device));
    RT_HIP(o, hipMemcpyAsync(dst, src, n_floats * sizeof(float), to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, on->stream));
    RT_HIP(o, hipStreamSynchronize(on->stream));
    return 0;
}

// The display step: linear -> sRGB8 of a plane of n_pixels > 0 on c's device (already current), through `display` there, on c's stream;
// kernel_ms, if asked for, is the kernel's time
hipError_t rth::display_plane(rt_ctx* c, const float4* plane, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels, float* kernel_ms)
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
int rth::read_srgb8(ErrOwner* o, rt_ctx* on, const float4* plane, size_t pixels, DevBuf<uint32_t>& display, uint32_t* rgba8, size_t n_pixels)
{
    if (n_pixels != pixels) return fail(o, -2, "expected %zu pixels (height*width), got %zu", pixels, n_pixels);
    if (!n_pixels) return 0;
    if (!plane) return fail(o, -2, "nothing rendered yet");
    RT_HIP(o, hipSetDevice(on->device));
    RT_HIP(o, display_plane(on, plane, display, rgba8, n_pixels));
    return 0;
}

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
    else if (!std::strcmp(name, "closest_box")) {
        if (value != 0 && value != 1) return fail(c, -2, "closest_box must be 0 or 1");
        if (value == 1 && c->opt_closest_capsule) return fail(c, -2, "closest_box cannot be 1 while closest_capsule is 1 (an input is a box or a segment)");
        c->opt_closest_box = value;
    }
    else if (!std::strcmp(name, "closest_capsule")) {
        if (value != 0 && value != 1) return fail(c, -2, "closest_capsule must be 0 or 1");
        if (value == 1 && c->opt_closest_box) return fail(c, -2, "closest_capsule cannot be 1 while closest_box is 1 (an input is a box or a segment)");
        c->opt_closest_capsule = value;
    }
    else if (!std::strcmp(name, "sweep")) { if (value != 0 && value != 1) return fail(c, -2, "sweep must be 0 or 1"); c->opt_sweep = value; }
    else if (!std::strcmp(name, "hits_sweep")) { if (value != 0 && value != 1) return fail(c, -2, "hits_sweep must be 0 or 1"); c->opt_hits_sweep = value; }
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

int rt_get_stats(rt_ctx* c, rt_stats* out)
{
    if (!c) return -1;
    RT_SETTLE(c);
    if (!out) return fail(c, -2, "null stats");
    *out = c->stats;
    return 0;
}

} // extern "C"
