// rt_query.hpp — ray queries: CalculateRayCollision (RayTracing.shader:256-297) for rays the caller supplies (include/rt.h rt_ray /
// rt_hit, rt_trace_rays / rt_occluded).
//
// One ray per lane, 256-thread blocks, one launch per batch (no persistent loop: every ray is one query).  The traversal stack is the
// renderer's: the first stack_cap entries per lane in LDS (stack[entry][lane]), deeper ones in the global overflow area, sized by the
// rule k_trace uses (rt_api.hip tile_stack_cap).
//   ANY = false   closest hit: closest_hit with best.t starting at the ray's tMax, mapped to the rt_hit record with the expressions
//                 render_pixel uses for hitPoint, normal and the chunk; the BVH-order triangle goes back to the uploaded one through the
//                 build's order map and, for local meshes, to its mesh.
//   ANY = true    occlusion: the first sphere or triangle with dst < tMax that the closest-hit query would accept ends the query.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 64, "a ray is two float4 loads, a hit four float4 stores");

struct QueryArgs {
    const float4* rays;         // [n*2]  rt_ray: (origin, tMax) (direction, -)
    float4* hits;               // [n*4]  rt_hit (closest hit)
    uint8_t* occluded;          // [n]    (occlusion)
    const uint32_t* order;      // BVH order -> uploaded triangle (d_order)
    const uint32_t* tri_mesh;   // uploaded triangle -> mesh (local uploads); null = world-space upload
    uint32_t* gstack;           // overflow of the traversal stack beyond stack_cap ([entry][lane of the launch]); may be null
    unsigned int gstack_stride; // lanes of the launch
    int n;
    int intersect_mode;
    int stack_cap;              // LDS stack entries per lane
    int full_sort;
};

// CalculateRayCollision with `dst < t_max` reduced to "is there a hit": every sphere first (no order matters for a yes / no), then the
// BVH with the slab test bounded by t_max.  A triangle counts when RayTriangle accepts it with dst < t_max and, in FLAT_CHUNKS mode, its
// chunk's RayBoundingBox passes (:279) — exactly the candidates closest_hit could take, so the answer is closest_hit's hit / miss.
// Returns the dst of the first accepted candidate (finite: it is < t_max), +inf when there is none.  (The answer is carried as that float,
// shaped like closest_hit — uniform scene test outside, divergent lane tests inside: a bool carried across the traversal became a lane
// mask that the uniform-region flags of the build merged wrongly, and lanes whose spheres had answered lost their yes.)
template <bool H>
__device__ __forceinline__ float any_hit(const DeviceScene& S, int intersect_mode, v3 o, v3 d, float t_max, const TravStack& stk)
{
    const float INF = __builtin_inff();
    const float a = rtm::dot(d, d);
    const SphereA sa = sphere_a(a);
    float hit_t = INF;
    for (int i = 0; i < S.ns; ++i) {
        const float4 s = S.sph_geom[i];
        float dst;
        if (ray_sphere(o, d, sa, rtm::mk(s.x, s.y, s.z), s.w, dst) && dst < t_max) hit_t = dst;
    }
    if (S.nn > 0 && ray_traceable(o, d, a)) {
        const RaySlabT<H> slab = make_slab<H>(o, d);
        int sp = 0;
        uint32_t cur = hit_t < INF ? kNone : 0u;                    // root, unless a sphere answered
        uint32_t top = kNone;                                       // the top of the stack in a register, as in closest_hit
#define RT_PUSH(X) { if (top != kNone) stk.push(sp, top); top = (X); }
#define RT_POP()   { cur = top; top = (sp > 0) ? stk.pop(sp) : kNone; }
        while (cur != kNone) {
            while ((int)cur >= 0) {
                float t0, t1, t2, t3;
                uint32_t c0, c1, c2, c3;
                node_step<H>(H ? S.nodes_h : S.nodes, cur, slab, t_max, false, t0, t1, t2, t3, c0, c1, c2, c3);
                if (t3 < INF) RT_PUSH(c3)
                if (t2 < INF) RT_PUSH(c2)
                if (t1 < INF) RT_PUSH(c1)
                if (t0 < INF) cur = c0;
                else RT_POP()
            }
            if (cur != kNone) {
                const uint32_t first = (cur & 0x7FFFFFFFu) >> 2, count = (cur & 3u) + 1u;
                for (uint32_t j = 0; j < count; ++j) {
                    const uint32_t ti = first + j;
                    float4 g0, g1, g2;
                    load_tri(S.tri_geo, ti, g0, g1, g2);
                    float dst, u, v;
                    if (ray_triangle(o, d, rtm::mk(g0.x, g0.y, g0.z), rtm::mk(g0.w, g1.x, g1.y), rtm::mk(g1.z, g1.w, g2.x), rtm::mk(g2.y, g2.z, g2.w),
                                     dst, u, v) && dst < t_max) {
                        bool take = true;
                        if (intersect_mode == RT_INTERSECT_FLAT_CHUNKS) {
                            // the reference only reaches this triangle if its chunk's box test passes (:279)
                            const uint32_t chunk = __float_as_uint(S.tri_nrm[(size_t)ti * 3].w);
                            const float4 bmn = S.chunk_box[(size_t)chunk * 2], bmx = S.chunk_box[(size_t)chunk * 2 + 1];
                            take = ray_bounding_box(o, slab.inv, rtm::mk(bmn.x, bmn.y, bmn.z), rtm::mk(bmx.x, bmx.y, bmx.z));
                        }
                        if (take) hit_t = dst;
                    }
                }
                if (hit_t < INF) cur = kNone;                       // the first accepted hit ends the query
                else RT_POP()
            }
        }
#undef RT_PUSH
#undef RT_POP
    }
    return hit_t;
}

template <bool ANY, bool H>
__global__ __launch_bounds__(kBlock) void k_ray_query(DeviceScene S, QueryArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float4 r0 = Q.rays[2 * (size_t)i], r1 = Q.rays[2 * (size_t)i + 1];
    const v3 o = rtm::mk(r0.x, r0.y, r0.z), d = rtm::mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w;
    const bool traced = t_max > 0.0f;                                   // tMax <= 0 or NaN: a miss, nothing traced
    if (ANY) {
        float hit_t = __builtin_inff();
        if (traced) hit_t = any_hit<H>(S, Q.intersect_mode, o, d, t_max, stk);
        Q.occluded[i] = hit_t < __builtin_inff() ? 1 : 0;
        return;
    }
    Hit h; h.id = kNone; h.t = __builtin_inff(); h.u = 0.f; h.v = 0.f;
    if (traced) {
        Counters cnt = {};
        h = closest_hit<false, H>(S, Q.intersect_mode, Q.full_sort != 0, o, d, stk, cnt, t_max);
    }
    float4 w0, w1, w2, w3;
    const float NEG1 = __int_as_float(-1), ZERO = 0.0f;
    if (h.id == kNone) {
        w0 = make_float4(__builtin_inff(), 0.f, 0.f, 0.f);
        w1 = make_float4(0.f, 0.f, 0.f, __int_as_float(RT_HIT_NONE));
        w2 = make_float4(NEG1, NEG1, NEG1, ZERO);
    } else {
        const v3 hitPoint = o + d * h.t;                                // render_pixel (Trace :309)
        v3 normal; const float4* mat;
        surface_of(S, h, hitPoint, normal, mat);
        if (h.id & kTriBit) {
            const uint32_t ti = h.id & ~kTriBit;
            const uint32_t prim = Q.order[ti];
            const int mesh = Q.tri_mesh ? (int)Q.tri_mesh[prim] : -1;
            w1 = make_float4(normal.x, normal.y, normal.z, __int_as_float(RT_HIT_TRIANGLE));
            w2 = make_float4(__uint_as_float(prim), S.tri_nrm[(size_t)ti * 3].w, __int_as_float(mesh), h.u);      // (.w: the chunk index's bits)
        } else {
            w1 = make_float4(normal.x, normal.y, normal.z, __int_as_float(RT_HIT_SPHERE));
            w2 = make_float4(__uint_as_float(h.id), NEG1, NEG1, ZERO);
        }
        w0 = make_float4(h.t, hitPoint.x, hitPoint.y, hitPoint.z);
    }
    w3 = make_float4(h.id != kNone && (h.id & kTriBit) ? h.v : ZERO, 0.f, 0.f, 0.f);
    float4* out = Q.hits + 4 * (size_t)i;
    out[0] = w0; out[1] = w1; out[2] = w2; out[3] = w3;
}

// Largest finite |origin coordinate| over the rays a query traces (tMax > 0): the box padding must cover it (bvh.cpp pad_box).  Non-negative
// floats order as their bit patterns, so the maximum is one integer atomic per wave.
template <int = 0>
__global__ __launch_bounds__(256) void k_query_origin_bound(const float4* __restrict__ rays, int n, unsigned int* __restrict__ bound)
{
    unsigned int m = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 r0 = rays[2 * i];
        if (!(r0.w > 0.0f)) continue;
        const float c[3] = { __builtin_fabsf(r0.x), __builtin_fabsf(r0.y), __builtin_fabsf(r0.z) };
        for (int a = 0; a < 3; ++a)
            if (c[a] <= 3.4028235e38f) m = max(m, __float_as_uint(c[a]));       // (finite only: NaN and inf fail the test)
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_down((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(bound, m);
}

} // namespace rtk
