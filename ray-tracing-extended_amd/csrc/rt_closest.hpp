// rt_closest.hpp — closest-point queries: the nearest surface to a POINT the caller supplies, how far away it is and on which side of
// it the point lies (include/rt.h rt_closest, rt_closest_points).  Signed-distance baking, probe placement, snapping, proximity tests.
// Geometry only: no rt_params field is read and nothing is shaded.
//
// Definition (include/rt.h "closest-point queries"; tests/closest_oracle.c restates it as a brute-force loop): every sphere and every
// triangle of the tree gets a float32 key k, its squared distance, every product and sum rounded on its own; a candidate counts when
// k < R * R and the smallest (k, kind, uploaded index) wins — whatever the tree, the builder, the leaf size or the visiting order.
//
// k_ray_query's launch: one point per lane, 256-thread blocks, one launch per slice, lane_stack's LDS stack with the global overflow.
// The traversal is ordered by distance, not by a slab test: a node step computes, for each of the four children,
//     lb2 = sum over the axes of max(lo - p, p - hi, 0)^2
// visits the nearest child next and pushes the others, farthest first.  A child is skipped only when lb2 > kb * (1 + 2^-19), kb the
// best key so far (R * R at the start): DESIGN.md "Closest-point queries" derives that this never skips a triangle whose key could
// count, equal keys included (a tie can still win on its index).  Entries already on the stack are not culled again when they are
// popped: a stale internal node costs one node step whose children are all skipped, a stale leaf its triangle tests.
// Shared: a node step's child boxes and sort (child_boxes, sort_children: rt_kernels.hpp, sweep_node_step's too); with the listed
// queries (rt_listed.hpp) child_gap2, closest_node_step, point_query, sphere_key, closest_triangle_record / closest_sphere_record,
// add_wave_counts, all below.
#pragma once
#include "rt_query.hpp"

namespace rtk {

static_assert(sizeof(rt_closest) == 64, "a closest-point record is four float4 stores");

struct ClosestArgs : QueryHead {        // (intersect_mode is not read: the chunk filter is a ray's)
    float4* out;                // [n*4]  rt_closest
    unsigned long long* counters;   // counting build: [0] node steps, [1] primitive tests (spheres and triangles) of the call so far
};

// kb * kCullSlack is the largest lower bound that is still visited; never below kCullFloor, so that no square that matters to the
// comparison is a denormal
constexpr float kCullSlack = 1.0f + 0x1p-19f;
constexpr float kCullFloor = 0x1p-100f;

// The closest point of triangle (A, A + ab, A + ac) to p as (u, v), point = A + ab * u + ac * v: the seven-region test (Ericson,
// Real-Time Collision Detection 5.1.5) on A, ab, ac and ap = p - A alone, in the operation order include/rt.h freezes.  The regions are
// tested in the order A, B, AB, C, AC, BC, interior; here the first that holds is picked by selects, and ONE quotient per coordinate is
// taken from the numerator and denominator that region names (a vertex: 0 / 1 or 1 / 1, exact).  Every comparison with a NaN is false,
// so a NaN anywhere ends in the interior formula and a NaN key, which never counts.
__device__ __forceinline__ void closest_on_triangle(v3 p, v3 A, v3 ab, v3 ac, float& k, float& u, float& v)
{
    const v3 ap = p - A;
    const float d1 = rtm::dot(ab, ap), d2 = rtm::dot(ac, ap);
    const v3 bp = ap - ab;
    const float d3 = rtm::dot(ab, bp), d4 = rtm::dot(ac, bp);
    const v3 cp = ap - ac;
    const float d5 = rtm::dot(ab, cp), d6 = rtm::dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const float den = (va + vb) + vc;
    const bool rA = d1 <= 0.0f && d2 <= 0.0f;
    const bool rB = d3 >= 0.0f && d4 <= d3;
    const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool rC = d6 >= 0.0f && d5 <= d6;
    const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool rBC = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
    // lowest priority first, each earlier region overriding the later ones
    float un = vb, ud = den, vn = vc, vd = den;                             // interior
    if (rBC) { un = 0.0f; ud = 1.0f; vn = d43; vd = d43 + d56; }            // (u = 1 - v below)
    if (rAC) { un = 0.0f; ud = 1.0f; vn = d2; vd = d2 - d6; }
    if (rC)  { un = 0.0f; ud = 1.0f; vn = 1.0f; vd = 1.0f; }
    if (rAB) { un = d1; ud = d1 - d3; vn = 0.0f; vd = 1.0f; }
    if (rB)  { un = 1.0f; ud = 1.0f; vn = 0.0f; vd = 1.0f; }
    if (rA)  { un = 0.0f; ud = 1.0f; vn = 0.0f; vd = 1.0f; }
    const bool edge_bc = rBC && !(rA || rB || rAB || rC || rAC);
    const bool interior = !(rA || rB || rAB || rC || rAC || rBC);
    u = un / ud;
    v = vn / vd;
    if (edge_bc) u = 1.0f - v;
    if (interior) {
        // rounding in va, vb, vc can leave the quotients just outside the triangle: bring them back (selects: a NaN stays a NaN)
        u = u < 0.0f ? 0.0f : u;
        u = u > 1.0f ? 1.0f : u;
        v = v < 0.0f ? 0.0f : v;
        const float room = 1.0f - u;
        v = v > room ? room : v;
    }
    const v3 q = (A + ab * u) + ac * v;
    const v3 e = p - q;
    k = rtm::dot(e, e);
}

// The squared lower bounds of the distance between the box [lo, hi] and each of the four child boxes: per axis
// max(child lo - hi, lo - child hi, 0), the squares summed as (x + y) + z.  A point is the box lo = hi = p.
__device__ __forceinline__ void child_gap2(const ChildBoxes& b, v3 lo, v3 hi, float& l0, float& l1, float& l2, float& l3)
{
#define RT_LB(K, LK)                                                                                                     \
    {                                                                                                                    \
        const float dx_ = __builtin_fmaxf(__builtin_fmaxf(b.lox.K - hi.x, lo.x - b.hix.K), 0.0f);                        \
        const float dy_ = __builtin_fmaxf(__builtin_fmaxf(b.loy.K - hi.y, lo.y - b.hiy.K), 0.0f);                        \
        const float dz_ = __builtin_fmaxf(__builtin_fmaxf(b.loz.K - hi.z, lo.z - b.hiz.K), 0.0f);                        \
        LK = (dx_ * dx_ + dy_ * dy_) + dz_ * dz_;                                                                        \
    }
    RT_LB(x, l0) RT_LB(y, l1) RT_LB(z, l2) RT_LB(w, l3)
#undef RT_LB
}

// The four children of node `cur`: their squared lower bounds from the box [lo, hi] (a point: lo = hi = p; a segment: its bounds,
// rt_capsule.hpp) sorted ascending with their references; a child that is empty or whose bound exceeds thr carries kNone (and +inf).
// The boxes are child_boxes' (rt_kernels.hpp).
template <bool H>
__device__ __forceinline__ void closest_node_step(const float4* __restrict__ nodes, uint32_t cur, v3 lo, v3 hi, float thr,
                                                  float& l0, float& l1, float& l2, float& l3,
                                                  uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3)
{
    const float INF = __builtin_inff();
    const ChildBoxes b = child_boxes<H>(nodes, cur);
    c0 = b.ch.x; c1 = b.ch.y; c2 = b.ch.z; c3 = b.ch.w;
    child_gap2(b, lo, hi, l0, l1, l2, l3);
    // an empty slot holds a (+inf, -inf) box: its bound is +inf, which is not above a threshold of +inf — it is dropped by its reference
    if (c0 == kNone || l0 > thr) { c0 = kNone; l0 = INF; }
    if (c1 == kNone || l1 > thr) { c1 = kNone; l1 = INF; }
    if (c2 == kNone || l2 > thr) { c2 = kNone; l2 = INF; }
    if (c3 == kNone || l3 > thr) { c3 = kNone; l3 = INF; }
    // sorted by (bound, dropped last): a kept child can have a bound of +inf too (thr = +inf, a point so far away that the squares
    // overflow), so the reference breaks the tie
    sort_children<true>(l0, l1, l2, l3, c0, c1, c2, c3);
}

// ---- what k_closest and the listed queries (rt_listed.hpp) share ----
// (p, R) of point i.  R <= 0 or NaN: not searched.  A point with a component that is not finite has no candidate either — every key it
// forms is +inf or NaN, and neither is below R * R — so it is answered without a search (its bounds would be +inf or NaN at every node)
struct PointQuery { v3 p; float R; bool searched; };
__device__ __forceinline__ PointQuery point_query(const float4* __restrict__ in, unsigned int i, bool present)
{
    const float FMAX = 3.4028235e38f;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (present) r0 = in[2 * (size_t)i];
    PointQuery q{ rtm::mk(r0.x, r0.y, r0.z), r0.w, false };
    q.searched = present && q.R > 0.0f && __builtin_fabsf(q.p.x) <= FMAX && __builtin_fabsf(q.p.y) <= FMAX && __builtin_fabsf(q.p.z) <= FMAX;
    return q;
}

// The key of scene sphere sp = (centre, radius): the squared distance from p to its surface
__device__ __forceinline__ float sphere_key(v3 p, float4 sp)
{
    const v3 m = p - rtm::mk(sp.x, sp.y, sp.z);
    const float len = rtm::sqrt_(rtm::dot(m, m));
    const float ds = __builtin_fabsf(len - sp.w);
    return ds * ds;
}

// The record of a winner, one function per kind, each called from the kernel's own `if (id & kTriBit)`: one function that branches
// on the id cost k_multihit up to 0.8 % (profiles/walk_refactor_timing.txt).
// BVH-order triangle ti at (u, v) with key `key`: the point again from (u, v), the same operations as in the search, the same bits
__device__ __forceinline__ HitRecord closest_triangle_record(const DeviceScene& S, const QueryHead& Q, v3 p, uint32_t ti, float u, float v,
                                                             float key, int count)
{
    float4 g0, g1, g2;
    load_tri(S.tri_geo, ti, g0, g1, g2);
    const v3 point = (rtm::mk(g0.x, g0.y, g0.z) + rtm::mk(g0.w, g1.x, g1.y) * u) + rtm::mk(g1.z, g1.w, g2.x) * v;
    const float s = rtm::dot(p - point, rtm::mk(g2.y, g2.z, g2.w));        // (n = cross(eAB, eAC), formed at the upload)
    const float dst = rtm::sqrt_(key);
    Hit h; h.id = kTriBit | ti; h.t = 0.0f; h.u = u; h.v = v;
    v3 normal; const float4* mat;
    surface_of(S, h, point, normal, mat);
    HitRecord rec;
    rec.triangle(S, Q, ti, normal, u, v, s > 0.0f ? 1 : s < 0.0f ? -1 : 0, count);
    rec.at(dst, point);
    return rec;
}
// scene sphere si
__device__ __forceinline__ HitRecord closest_sphere_record(const DeviceScene& S, v3 p, uint32_t si, int count)
{
    const float4 sp = S.sph_geom[si];
    const v3 c = rtm::mk(sp.x, sp.y, sp.z), m = p - c;
    const float len = rtm::sqrt_(rtm::dot(m, m));
    const float dst = __builtin_fabsf(len - sp.w);
    const v3 point = c + m * (sp.w / len);
    Hit h; h.id = si; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f;
    v3 normal; const float4* mat;
    surface_of(S, h, point, normal, mat);
    HitRecord rec;
    rec.sphere(si, normal, len >= sp.w ? 1 : -1, count);
    rec.at(dst, point);
    return rec;
}

// The counting build's tail: the wave's sums of node steps and primitive tests, one pair of atomics per wave (every lane takes part)
__device__ __forceinline__ void add_wave_counts(unsigned long long* counters, uint32_t n_nodes, uint32_t n_prims)
{
    unsigned long long a = n_nodes, b = n_prims;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&counters[0], a); atomicAdd(&counters[1], b); }
}

template <bool H, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_closest(DeviceScene S, ClosestArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    const bool present = i < (unsigned)Q.n;
    if (!COUNT && !present) return;                                     // (the counting build keeps every lane for the wave's sums)
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const PointQuery q = point_query(Q.in, i, present);
    const v3 p = q.p;
    float kb = q.R * q.R;                                               // the best key so far; before the first candidate, the bound
    uint32_t best = kNone;                                              // kNone | sphere index | kTriBit + triangle in BVH order
    float bu = 0.0f, bv = 0.0f;
    uint32_t n_nodes = 0, n_prims = 0;

    if (q.searched) {
        for (int s = 0; s < S.ns; ++s) {
            const float k = sphere_key(p, S.sph_geom[s]);
            if (COUNT) ++n_prims;
            if (k < kb) { kb = k; best = (uint32_t)s; }                // strict: the lower index keeps a tie
        }
        if (S.nn > 0) {
            const float4* nodes = H ? S.nodes_h : S.nodes;
            RT_WALK_NODE(stk, 0u)                                       // from the root
                if (COUNT) ++n_nodes;
                float l0, l1, l2, l3;
                uint32_t c0, c1, c2, c3;
                closest_node_step<H>(nodes, node, p, p, __builtin_fmaxf(kb * kCullSlack, kCullFloor), l0, l1, l2, l3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, c0 != kNone, c1 != kNone, c2 != kNone, c3 != kNone)
                float k, u, v;
                closest_on_triangle(p, tri_A, tri_AB, tri_AC, k, u, v);
                if (COUNT) ++n_prims;
                if (k <= kb) {
                    bool take = k < kb;
                    // equal keys: a sphere keeps the tie (and so does the bound R * R while nothing has been found); between
                    // triangles the lower uploaded index wins
                    if (!take && best != kNone && (best & kTriBit)) take = Q.order[ti] < Q.order[best & ~kTriBit];
                    if (take) { kb = k; best = kTriBit | ti; bu = u; bv = v; }
                }
            RT_WALK_END(false)
        }
    }

    if (present) {
        HitRecord rec;
        if (best == kNone) rec.miss(0);
        else if (best & kTriBit) rec = closest_triangle_record(S, Q, p, best & ~kTriBit, bu, bv, kb, 0);
        else rec = closest_sphere_record(S, p, best, 0);
        rec.store(Q.out + 4 * (size_t)i);
    }
    if (COUNT) add_wave_counts(Q.counters, n_nodes, n_prims);
}

} // namespace rtk
