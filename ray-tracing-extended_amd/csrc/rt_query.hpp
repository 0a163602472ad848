// rt_query.hpp — ray queries: CalculateRayCollision (RayTracing.shader:256-297) for rays the caller supplies (include/rt.h rt_ray /
// rt_hit, rt_trace_rays / rt_occluded).
//
// One ray per lane, 256-thread blocks, one launch per batch (no persistent loop: every ray is one query).  The traversal stack is the
// renderer's: the first stack_cap entries per lane in LDS (stack[entry][lane]), deeper ones in the global overflow area, sized by the
// rule k_trace uses (rt_api.hip tile_stack_cap, plan_lane_stack).
//   ANY = false   closest hit: closest_hit with best.t starting at the ray's tMax, mapped to the rt_hit record with the expressions
//                 render_pixel uses for hitPoint, normal and the chunk; the BVH-order triangle goes back to the uploaded one through the
//                 build's order map and, for local meshes, to its mesh.
//   ANY = true    occlusion: the first sphere or triangle with dst < tMax that the closest-hit query would accept ends the query.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 64, "a ray is two float4 loads, a hit four float4 stores");

// What the kernels that answer with a HitRecord take, first: k_multihit (rt_multihit.hpp), k_closest (rt_closest.hpp)
struct QueryHead {
    const float4* in;           // [n*2]  rt_ray: (origin, tMax) (direction, -); closest-point queries: (p, R) (-, -)
    const uint32_t* order;      // BVH order -> uploaded triangle (d_order)
    const uint32_t* tri_mesh;   // uploaded triangle -> mesh (local uploads); null = world-space upload
    uint32_t* gstack;           // overflow of the traversal stack beyond stack_cap ([entry][lane of the launch]); may be null
    unsigned int gstack_stride; // lanes of the launch
    int n;
    int intersect_mode;
    int stack_cap;              // LDS stack entries per lane
};

// k_ray_query's: the head's fields under the head's names, in the order this kernel was measured with — with QueryHead first and its
// record written by HitRecord the closest-hit form ran 1 % slower (profiles/walk_refactor_timing.txt), so it keeps both as they were
struct QueryArgs {
    const float4* in;           // [n*2]  rt_ray
    float4* hits;               // [n*4]  rt_hit (closest hit)
    uint8_t* occluded;          // [n]    (occlusion)
    const uint32_t* order;
    const uint32_t* tri_mesh;
    uint32_t* gstack;
    unsigned int gstack_stride;
    int n;
    int intersect_mode;
    int stack_cap;
    int full_sort;
};

// CalculateRayCollision with `dst < t_max` reduced to "is there a hit": every sphere first (no order matters for a yes / no), then the
// BVH with the slab test bounded by t_max.  A triangle counts when RayTriangle accepts it with dst < t_max and, in FLAT_CHUNKS mode, its
// chunk's RayBoundingBox passes (:279) — exactly the candidates closest_hit could take, so the answer is closest_hit's hit / miss.
// Returns the dst of the first accepted candidate (finite: it is < t_max), +inf when there is none: the answer crosses the walk as
// that float, never as a bool (rt_kernels.hpp, the per-lane walk).
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
        RT_WALK_NODE(stk, hit_t < INF ? kNone : 0u)                     // from the root, unless a sphere answered
            float t0, t1, t2, t3;
            uint32_t c0, c1, c2, c3;
            node_step<H>(H ? S.nodes_h : S.nodes, node, slab, t_max, false, t0, t1, t2, t3, c0, c1, c2, c3);
        RT_WALK_TRIANGLE(S.tri_geo, t0 < INF, t1 < INF, t2 < INF, t3 < INF)
            float dst, u, v;
            if (ray_triangle(o, d, tri_A, tri_AB, tri_AC, tri_n, dst, u, v) && dst < t_max) {
                bool take = true;
                if (intersect_mode == RT_INTERSECT_FLAT_CHUNKS) take = chunk_passes(S, ti, o, slab.inv);
                if (take) hit_t = dst;
            }
        RT_WALK_END(hit_t < INF)                                        // the first accepted hit ends the query
    }
    return hit_t;
}

// The record rt_hit, rt_multihit and rt_closest share, four float4 stores: w0 = dst + point, w1 = normal + kind, w2 = primitive / chunk
// index's bits / mesh / u, w3 = v / side / count / 0.  One of the three forms fills it, then store() writes it.  normal is Trace's
// (surface_of).  k_multihit and k_closest write theirs with it; k_ray_query's epilogue is its own (QueryArgs).
struct HitRecord {
    float4 w0, w1, w2, w3;
    __device__ __forceinline__ void miss(int count)
    {
        const float NEG1 = __int_as_float(-1);
        w0 = make_float4(__builtin_inff(), 0.f, 0.f, 0.f);
        w1 = make_float4(0.f, 0.f, 0.f, __int_as_float(RT_HIT_NONE));
        w2 = make_float4(NEG1, NEG1, NEG1, 0.f);
        w3 = make_float4(0.f, __int_as_float(0), __int_as_float(count), 0.f);
    }
    // (a sphere or a triangle: w1 .. w3 here, w0 by at())
    __device__ __forceinline__ void sphere(uint32_t index, v3 normal, int side, int count)
    {
        const float NEG1 = __int_as_float(-1);
        w1 = make_float4(normal.x, normal.y, normal.z, __int_as_float(RT_HIT_SPHERE));
        w2 = make_float4(__uint_as_float(index), NEG1, NEG1, 0.f);
        w3 = make_float4(0.f, __int_as_float(side), __int_as_float(count), 0.f);
    }
    // BVH-order triangle ti: back to the uploaded one through the build's order map and, for local meshes, to its mesh
    __device__ __forceinline__ void triangle(const DeviceScene& S, const QueryHead& Q, uint32_t ti, v3 normal, float u, float v, int side, int count)
    {
        const uint32_t prim = Q.order[ti];
        const int mesh = Q.tri_mesh ? (int)Q.tri_mesh[prim] : -1;
        w1 = make_float4(normal.x, normal.y, normal.z, __int_as_float(RT_HIT_TRIANGLE));
        w2 = make_float4(__uint_as_float(prim), S.tri_nrm[(size_t)ti * 3].w, __int_as_float(mesh), u);      // (.w: the chunk index's bits)
        w3 = make_float4(v, __int_as_float(side), __int_as_float(count), 0.f);
    }
    __device__ __forceinline__ void at(float dst, v3 point) { w0 = make_float4(dst, point.x, point.y, point.z); }
    __device__ __forceinline__ void store(float4* out) const { out[0] = w0; out[1] = w1; out[2] = w2; out[3] = w3; }
};

template <bool ANY, bool H>
__global__ __launch_bounds__(kBlock) void k_ray_query(DeviceScene S, QueryArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float4 r0 = Q.in[2 * (size_t)i], r1 = Q.in[2 * (size_t)i + 1];
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
// ENDS = 1 (capsule overlap queries, rt_capsule.hpp): an input is a segment, and its other endpoint origin + direction counts as well.
template <int ENDS = 0>
__global__ __launch_bounds__(256) void k_query_origin_bound(const float4* __restrict__ rays, int n, unsigned int* __restrict__ bound)
{
    unsigned int m = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 r0 = rays[2 * i];
        if (!(r0.w > 0.0f)) continue;
        const float c[3] = { __builtin_fabsf(r0.x), __builtin_fabsf(r0.y), __builtin_fabsf(r0.z) };
        for (int a = 0; a < 3; ++a)
            if (c[a] <= 3.4028235e38f) m = max(m, __float_as_uint(c[a]));       // (finite only: NaN and inf fail the test)
        if constexpr (ENDS != 0) {
            const float4 r1 = rays[2 * i + 1];
            const float e[3] = { __builtin_fabsf(r0.x + r1.x), __builtin_fabsf(r0.y + r1.y), __builtin_fabsf(r0.z + r1.z) };
            for (int a = 0; a < 3; ++a)
                if (e[a] <= 3.4028235e38f) m = max(m, __float_as_uint(e[a]));
        }
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_down((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(bound, m);
}

} // namespace rtk
