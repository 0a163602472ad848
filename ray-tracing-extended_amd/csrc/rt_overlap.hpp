// rt_overlap.hpp — box overlap queries: EVERY surface that touches an axis-aligned box the caller supplies, nearest to the box's centre
// first, and how many there are (include/rt.h "box overlap queries": option "closest_box" of rt_closest_points): Unity's
// Physics.OverlapBox / CheckBox beside OverlapSphere, and conservative voxelisation with one box per cell.
//
// Definition (tests/overlap_oracle.c restates it as a brute-force loop and a sort): the closest-point queries' candidates; a candidate
// counts when it TOUCHES the closed box [c - h, c + h] — a solid scene sphere by its distance to the box, a triangle by the 13-axis
// separating-axis test (Akenine-Möller) after a finiteness and a bounds condition — and its closest-point key from the centre c is not
// NaN.  There is no radius.  Records, order and count are the K-nearest queries' (rt_nearest.hpp), the keys taken from c.
//
// The listed-query frame (rt_listed.hpp) and k_nearest's keys and record writers, with two pieces of its own: box_touches_triangle, and
// a node step that takes closest_node_step's sorted lower bounds from c and also drops every child whose box is disjoint from [lo, hi]
// by exact comparison.
//
// Pruning.  A child is skipped when its box misses [lo, hi] on some axis: a touching triangle passes the bounds condition on A, A + eAB,
// A + eAC, and those bounds lie inside every box on the way down to it (DESIGN.md "Box overlap queries").  Without closest_all a child is
// also skipped when lb2 > max(kth * kCullSlack, kCullFloor), kth the key in slot K - 1: the K-nearest rule, on the subset that touches.
#pragma once
#include "rt_listed.hpp"

namespace rtk {

// (c, h) of box i, and lo = c - h, hi = c + h.  tMax is only a gate: <= 0 or NaN, a centre or a half-extent that is not finite, or a
// negative half-extent: not searched
struct BoxQuery { v3 c, h, lo, hi; bool searched; };
__device__ __forceinline__ BoxQuery box_query(const float4* __restrict__ in, unsigned int i, bool present)
{
    const float FMAX = 3.4028235e38f;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (present) { r0 = in[2 * (size_t)i]; r1 = in[2 * (size_t)i + 1]; }
    BoxQuery q;
    q.c = rtm::mk(r0.x, r0.y, r0.z);
    q.h = rtm::mk(r1.x, r1.y, r1.z);
    q.lo = q.c - q.h;
    q.hi = q.c + q.h;
    q.searched = present && r0.w > 0.0f && __builtin_fabsf(q.c.x) <= FMAX && __builtin_fabsf(q.c.y) <= FMAX && __builtin_fabsf(q.c.z) <= FMAX
              && q.h.x >= 0.0f && q.h.y >= 0.0f && q.h.z >= 0.0f && q.h.x <= FMAX && q.h.y <= FMAX && q.h.z <= FMAX;
    return q;
}

// A solid scene sphere sp = (centre, radius) touches the box when the squared distance from its centre to the box is <= radius^2
__device__ __forceinline__ bool box_touches_sphere(const BoxQuery& q, float4 sp)
{
    const float ex = __builtin_fmaxf(__builtin_fmaxf(q.lo.x - sp.x, sp.x - q.hi.x), 0.0f);
    const float ey = __builtin_fmaxf(__builtin_fmaxf(q.lo.y - sp.y, sp.y - q.hi.y), 0.0f);
    const float ez = __builtin_fmaxf(__builtin_fmaxf(q.lo.z - sp.z, sp.z - q.hi.z), 0.0f);
    const float d2 = (ex * ex + ey * ey) + ez * ez;
    return d2 <= sp.w * sp.w;
}

// Triangle (A, A + eAB, A + eAC) against the closed box: the header's four conditions, every comparison false for a NaN.  n is
// cross(eAB, eAC) as the upload formed it.  No early exit: the conditions are combined with &, one verdict at the end (an exit after the
// bounds condition cost 13 VGPRs, 98 against 85, and the fifth wave per SIMD: profiles/overlap_timing.txt).
__device__ __forceinline__ bool box_touches_triangle(const BoxQuery& q, v3 A, v3 eAB, v3 eAC, v3 n)
{
    const v3 B = A + eAB, C = A + eAC;
    const float BIG = 1e30f;
    int ok = (__builtin_fabsf(A.x) < BIG) & (__builtin_fabsf(A.y) < BIG) & (__builtin_fabsf(A.z) < BIG)
           & (__builtin_fabsf(B.x) < BIG) & (__builtin_fabsf(B.y) < BIG) & (__builtin_fabsf(B.z) < BIG)
           & (__builtin_fabsf(C.x) < BIG) & (__builtin_fabsf(C.y) < BIG) & (__builtin_fabsf(C.z) < BIG);
#define RT_BOUNDS(a) ok &= (__builtin_fminf(__builtin_fminf(A.a, B.a), C.a) <= q.hi.a) & (__builtin_fmaxf(__builtin_fmaxf(A.a, B.a), C.a) >= q.lo.a);
    RT_BOUNDS(x) RT_BOUNDS(y) RT_BOUNDS(z)
#undef RT_BOUNDS
    const v3 h = q.h;
    const v3 v0 = A - q.c, v1 = B - q.c, v2 = C - q.c;
    const float d = rtm::dot(n, v0);
    const float rr = (h.x * __builtin_fabsf(n.x) + h.y * __builtin_fabsf(n.y)) + h.z * __builtin_fabsf(n.z);
    ok &= __builtin_fabsf(d) <= rr;
    // one edge f against one box axis: the three projections p_j = v_j.P * f.Q - v_j.Q * f.P, the radius r = h.Q * |f.P| + h.P * |f.Q|
    // written in the header's operand order by the callers below
#define RT_AXIS(P0, P1, P2, R)                                                                                           \
    {                                                                                                                    \
        const float p0_ = (P0), p1_ = (P1), p2_ = (P2), r_ = (R);                                                        \
        ok &= (__builtin_fminf(__builtin_fminf(p0_, p1_), p2_) <= r_) & (__builtin_fmaxf(__builtin_fmaxf(p0_, p1_), p2_) >= -r_); \
    }
#define RT_EDGE(f)                                                                                                       \
    RT_AXIS(v0.z * f.y - v0.y * f.z, v1.z * f.y - v1.y * f.z, v2.z * f.y - v2.y * f.z, h.y * __builtin_fabsf(f.z) + h.z * __builtin_fabsf(f.y)) \
    RT_AXIS(v0.x * f.z - v0.z * f.x, v1.x * f.z - v1.z * f.x, v2.x * f.z - v2.z * f.x, h.x * __builtin_fabsf(f.z) + h.z * __builtin_fabsf(f.x)) \
    RT_AXIS(v0.y * f.x - v0.x * f.y, v1.y * f.x - v1.x * f.y, v2.y * f.x - v2.x * f.y, h.x * __builtin_fabsf(f.y) + h.y * __builtin_fabsf(f.x))
    const v3 f1 = eAC - eAB;
    RT_EDGE(eAB) RT_EDGE(f1) RT_EDGE(eAC)
#undef RT_EDGE
#undef RT_AXIS
    return ok != 0;
}

// A touching candidate's key, from the centre, counts unless it is NaN.  It can be +inf — a box far from the surface it still reaches —
// and then ties with the list's empty slots: insert<true> keeps the tie read off them, and the candidate goes in front of them, kNone
// being the largest id.
struct BoxShape : BoxQuery {
    static constexpr bool kInfKeys = true;
    static __device__ __forceinline__ BoxShape load(const float4* __restrict__ in, unsigned int i, bool present)
    {
        return BoxShape{ box_query(in, i, present) };
    }
    __device__ __forceinline__ bool admits(float k) const { return k == k; }
    __device__ __forceinline__ float threshold(bool count_all, float kth) const
    {
        return count_all ? __builtin_inff() : __builtin_fmaxf(kth * kCullSlack, kCullFloor);
    }
    // closest_node_step with one more reason to drop a child: its box misses [lo, hi] on some axis (exact comparisons; an empty slot's
    // (+inf, -inf) box misses everything).  The kept children come back sorted by their squared lower bound from c, nearest first.
    template <bool H>
    __device__ __forceinline__ void node_step(const float4* __restrict__ nodes, uint32_t cur, float thr, float& l0, float& l1, float& l2, float& l3,
                                              uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) const
    {
        const float INF = __builtin_inff();
        const ChildBoxes b = child_boxes<H>(nodes, cur);
        c0 = b.ch.x; c1 = b.ch.y; c2 = b.ch.z; c3 = b.ch.w;
        child_gap2(b, c, c, l0, l1, l2, l3);
#define RT_DROP(K, LK, CK)                                                                                               \
        {                                                                                                                \
            const bool apart_ = b.lox.K > hi.x || b.hix.K < lo.x || b.loy.K > hi.y || b.hiy.K < lo.y || b.loz.K > hi.z || b.hiz.K < lo.z; \
            if (CK == kNone || apart_ || LK > thr) { CK = kNone; LK = INF; }                                             \
        }
        RT_DROP(x, l0, c0) RT_DROP(y, l1, c1) RT_DROP(z, l2, c2) RT_DROP(w, l3, c3)
#undef RT_DROP
        sort_children<true>(l0, l1, l2, l3, c0, c1, c2, c3);
    }
    __device__ __forceinline__ bool sphere(float4 sp, float& k) const
    {
        if (!box_touches_sphere(*this, sp)) return false;
        k = sphere_key(c, sp);
        return true;
    }
    __device__ __forceinline__ bool triangle(v3 A, v3 AB, v3 AC, v3 n, float& k) const
    {
        if (!box_touches_triangle(*this, A, AB, AC, n)) return false;
        float u, v;
        closest_on_triangle(c, A, AB, AC, k, u, v);
        return true;
    }
    // k_nearest's records, from the centre
    __device__ __forceinline__ HitRecord triangle_record(const DeviceScene& S, const QueryHead& Q, uint32_t ti, v3 A, v3 AB, v3 AC, v3,
                                                         float key, int count) const
    {
        float k_again, u, v;
        closest_on_triangle(c, A, AB, AC, k_again, u, v);
        return closest_triangle_record(S, Q, c, ti, u, v, key, count);
    }
    __device__ __forceinline__ HitRecord sphere_record(const DeviceScene& S, uint32_t si, int count) const
    {
        return closest_sphere_record(S, c, si, count);
    }
};

template <bool H, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_overlap(DeviceScene S, NearestArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    listed_query<BoxShape, H, COUNT>(S, Q, lds_stack);
}

} // namespace rtk

