// rt_capsule.hpp — capsule overlap queries: EVERY surface within R of a SEGMENT the caller supplies, nearest first, where on the surface,
// where on the segment, and how many there are (include/rt.h "capsule overlap queries": option "closest_capsule" of rt_closest_points):
// Unity's Physics.OverlapCapsule / CheckCapsule beside OverlapSphere and OverlapBox; ropes, bones, depenetration, clearance along a move.
//
// Definition (tests/capsule_oracle.c restates it as a brute-force loop and a sort): an input is P0 = origin, d = direction, P1 = P0 + d,
// R = tMax.  The closest-point queries' candidates; a candidate's key k is the squared distance between a point x = P0 + d * s of the
// segment and a point of the surface — a triangle's the smallest of up to six sub-candidates formed in a fixed order (the two endpoints
// through closest_on_triangle, the three edges through the clamped segment-segment pair, the two-sided RayTriangle), a solid sphere's
// from the segment's point nearest to its centre.  It counts when k < R * R.  Records, order and count are the K-nearest queries'
// (rt_nearest.hpp); _reserved[1] of a record carries the bits of s.
//
// The listed-query frame (rt_listed.hpp) and k_closest's record writers with three pieces of its own: segment_query, segment_triangle /
// segment_sphere, and closest_node_step taken from the segment's own axis-aligned bounds: a child's lower bound is the squared distance
// between its box and them.  A listed winner's test is run again for its (s, u, v).
//
// Pruning.  kb as in k_nearest; a child is skipped only when lb2 > max(kb * kCullSlack, kCullFloor).  Every sub-candidate's key is
// |x - q|^2 of a COMPUTED x = fl(P0 + fl(d * s)), s in [0, 1], and a computed q on the triangle.  Rounding is monotone, so x lies in
// [min(P0, P1), max(P0, P1)] on every axis exactly, and q lies in the padded box as in the closest-point proof: the closest-point
// derivation holds with "the point" replaced by "the segment's bounds", and 2^-19 still suffices (DESIGN.md "Capsule overlap queries").
// That is why the piercing sub-candidate's key is |x - q|^2 of its own (t, u, v), 0 whenever the two coincide, and not a constant.
//
// Registers (tools/kernel_resources.py on the built code object): 89 VGPRs plain, 93 counting, both node forms; 78 / 80 SGPRs; no
// scratch, no spills in any of the four instantiations; five waves per SIMD, k_overlap's occupancy (k_nearest: 64 / 69, eight / seven).
// The six sub-candidates are evaluated one after the other into a running (k, s, u, v), not side by side.
#pragma once
#include "rt_listed.hpp"

namespace rtk {

// (P0, d, P1 = P0 + d, R) of segment i, the segment's bounds and dd = dot(d, d).  R <= 0 or NaN, or a component of P0, d or P1 that is not
// finite: not searched
struct SegmentQuery { v3 p0, d, p1, lo, hi; float R, dd; bool searched; };
__device__ __forceinline__ SegmentQuery segment_query(const float4* __restrict__ in, unsigned int i, bool present)
{
    const float FMAX = 3.4028235e38f;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (present) { r0 = in[2 * (size_t)i]; r1 = in[2 * (size_t)i + 1]; }
    SegmentQuery q;
    q.p0 = rtm::mk(r0.x, r0.y, r0.z);
    q.d = rtm::mk(r1.x, r1.y, r1.z);
    q.p1 = q.p0 + q.d;
    q.R = r0.w;
    q.dd = rtm::dot(q.d, q.d);
    q.lo = rtm::mk(__builtin_fminf(q.p0.x, q.p1.x), __builtin_fminf(q.p0.y, q.p1.y), __builtin_fminf(q.p0.z, q.p1.z));
    q.hi = rtm::mk(__builtin_fmaxf(q.p0.x, q.p1.x), __builtin_fmaxf(q.p0.y, q.p1.y), __builtin_fmaxf(q.p0.z, q.p1.z));
    q.searched = present && q.R > 0.0f
              && __builtin_fabsf(q.p0.x) <= FMAX && __builtin_fabsf(q.p0.y) <= FMAX && __builtin_fabsf(q.p0.z) <= FMAX
              && __builtin_fabsf(q.d.x) <= FMAX && __builtin_fabsf(q.d.y) <= FMAX && __builtin_fabsf(q.d.z) <= FMAX
              && __builtin_fabsf(q.p1.x) <= FMAX && __builtin_fabsf(q.p1.y) <= FMAX && __builtin_fabsf(q.p1.z) <= FMAX;
    return q;
}

// x < 0 ? 0 : x > 1 ? 1 : x — selects: a NaN stays a NaN
__device__ __forceinline__ float clamp01(float x)
{
    x = x < 0.0f ? 0.0f : x;
    return x > 1.0f ? 1.0f : x;
}

// The parameter of the segment's point nearest to c: clamp01(dot(c - P0, d) / dd), 0 for a point
__device__ __forceinline__ float segment_param(const SegmentQuery& q, v3 c)
{
    const float t = clamp01(rtm::dot(c - q.p0, q.d) / q.dd);
    return q.dd == 0.0f ? 0.0f : t;
}

// Solid scene sphere sp = (centre, radius): t = segment_param, x = P0 + d * t, m = x - c, len = |m|, ds = max(len - r, 0) by a select (a NaN
// stays a NaN), k = ds * ds
__device__ __forceinline__ float segment_sphere(const SegmentQuery& q, float4 sp, float& s, v3& m, float& len, float& ds)
{
    const v3 c = rtm::mk(sp.x, sp.y, sp.z);
    s = segment_param(q, c);
    const v3 x = q.p0 + q.d * s;
    m = x - c;
    len = rtm::sqrt_(rtm::dot(m, m));
    ds = len - sp.w;
    ds = ds < 0.0f ? 0.0f : ds;
    return ds * ds;
}

// The clamped closest pair of the segment and the edge E0 + e * t, t in [0, 1] (Ericson, Real-Time Collision Detection 5.1.9), called
// with dd > 0 only.  In the header's operation order:
//     r = P0 - E0;  ee = dot(e, e);  f = dot(e, r);  c = dot(d, r);  b = dot(d, e);  den = dd * ee - b * b
//     s0 = den > 0 ? clamp01((b * f - c * ee) / den) : 0                   (parallel, or den rounded to <= 0: any s serves)
//     t0 = (b * s0 + f) / ee
//     below = ee == 0 || t0 < 0;  above = !below && t0 > 1                 (a degenerate edge is its point E0: t = 0)
//     t = below ? 0 : above ? 1 : t0
//     s = below ? clamp01(-c / dd) : above ? clamp01((b - c) / dd) : s0
// A NaN t0 is neither below nor above and ends in a NaN key, which never replaces anything.
__device__ __forceinline__ void segment_edge(const SegmentQuery& q, v3 E0, v3 e, float& s, float& t)
{
    const v3 r = q.p0 - E0;
    const float ee = rtm::dot(e, e), f = rtm::dot(e, r), c = rtm::dot(q.d, r), b = rtm::dot(q.d, e);
    const float den = q.dd * ee - b * b;
    const float s0 = den > 0.0f ? clamp01((b * f - c * ee) / den) : 0.0f;
    const float t0 = (b * s0 + f) / ee;
    const bool below = ee == 0.0f || t0 < 0.0f;
    const bool above = !below && t0 > 1.0f;
    const float sn = below ? -c : b - c;
    const float s1 = clamp01(sn / q.dd);
    t = below ? 0.0f : above ? 1.0f : t0;
    s = (below || above) ? s1 : s0;
}

// The key of triangle (A, A + ab, A + ac), n = cross(ab, ac): the smallest of the sub-candidates, formed in the order endpoint P0,
// endpoint P1, edge AB, edge AC, edge BC, piercing, each into the running (k, s, u, v); a later one replaces the running best only when
// its key is strictly smaller (a NaN never does).  pierced: the piercing sub-candidate is the one that stands.
// An edge sub-candidate reports closest_on_triangle's edge coordinates — AB (t, 0), AC (0, t), BC (1 - t, t) — and every sub-candidate
// but the endpoints' forms its key the same way: x = P0 + d * s, q = (A + ab * u) + ac * v, k = dot(x - q, x - q).
__device__ __forceinline__ void segment_triangle(const SegmentQuery& q, v3 A, v3 ab, v3 ac, v3 n, float& k, float& s, float& u, float& v, bool& pierced)
{
    closest_on_triangle(q.p0, A, ab, ac, k, u, v);
    s = 0.0f;
    pierced = false;
    if (q.dd != 0.0f) {
        {
            float k2, u2, v2;
            closest_on_triangle(q.p1, A, ab, ac, k2, u2, v2);
            if (k2 < k) { k = k2; s = 1.0f; u = u2; v = v2; }
        }
#define RT_PAIR(S_, U_, V_, FLAG_)                                                                                      \
        {                                                                                                                \
            const float cs_ = (S_), cu_ = (U_), cv_ = (V_);                                                              \
            const v3 x_ = q.p0 + q.d * cs_;                                                                              \
            const v3 y_ = (A + ab * cu_) + ac * cv_;                                                                     \
            const v3 e_ = x_ - y_;                                                                                       \
            const float ck_ = rtm::dot(e_, e_);                                                                          \
            if (ck_ < k) { k = ck_; s = cs_; u = cu_; v = cv_; pierced = (FLAG_); }                                      \
        }
        float es, et;
        segment_edge(q, A, ab, es, et);
        RT_PAIR(es, et, 0.0f, false)
        segment_edge(q, A, ac, es, et);
        RT_PAIR(es, 0.0f, et, false)
        segment_edge(q, A + ab, ac - ab, es, et);
        RT_PAIR(es, 1.0f - et, et, false)
        float pt, pu, pv;
        const int side = ray_triangle_sided<true>(q.p0, q.d, A, ab, ac, n, pt, pu, pv);
        if (side != 0 && pt <= 1.0f) RT_PAIR(pt, pu, pv, true)
#undef RT_PAIR
    }
}

// (R * R can be +inf but a counted key is below it, so the keys offered are finite)
struct SegmentShape : WithinReach<SegmentQuery> {
    static __device__ __forceinline__ SegmentShape load(const float4* __restrict__ in, unsigned int i, bool present)
    {
        return SegmentShape{ { segment_query(in, i, present) } };
    }
    template <bool H>
    __device__ __forceinline__ void node_step(const float4* __restrict__ nodes, uint32_t cur, float thr, float& l0, float& l1, float& l2, float& l3,
                                              uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) const
    {
        closest_node_step<H>(nodes, cur, lo, hi, thr, l0, l1, l2, l3, c0, c1, c2, c3);
    }
    __device__ __forceinline__ bool sphere(float4 sp, float& k) const
    {
        float s, len, ds; v3 m;
        k = segment_sphere(*this, sp, s, m, len, ds);
        return true;
    }
    __device__ __forceinline__ bool triangle(v3 A, v3 AB, v3 AC, v3 n, float& k) const
    {
        float s, u, v; bool pierced;
        segment_triangle(*this, A, AB, AC, n, k, s, u, v, pierced);
        return true;
    }
    // k_closest's triangle record from x = P0 + d * s; the sphere record is the solid sphere's.  _reserved[1] (w3.w) carries the bits of s.
    __device__ __forceinline__ HitRecord triangle_record(const DeviceScene& S, const QueryHead& Q, uint32_t ti, v3 A, v3 AB, v3 AC, v3 n,
                                                         float key, int count) const
    {
        float k_again, s, u, v; bool pierced;
        segment_triangle(*this, A, AB, AC, n, k_again, s, u, v, pierced);
        HitRecord rec = closest_triangle_record(S, Q, p0 + d * s, ti, u, v, key, count);
        if (pierced) rec.w3.y = __int_as_float(0);                      // (a piercing segment lies on neither side)
        rec.w3.w = s;
        return rec;
    }
    __device__ __forceinline__ HitRecord sphere_record(const DeviceScene& S, uint32_t si, int count) const
    {
        const float4 sp = S.sph_geom[si];
        float s, len, ds; v3 m;
        segment_sphere(*this, sp, s, m, len, ds);
        const v3 c = rtm::mk(sp.x, sp.y, sp.z);
        const v3 point = c + m * (sp.w / len);
        Hit h; h.id = si; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f;
        v3 normal; const float4* mat;
        surface_of(S, h, point, normal, mat);
        HitRecord rec;
        rec.sphere(si, normal, len >= sp.w ? 1 : -1, count);
        rec.at(ds, point);
        rec.w3.w = s;
        return rec;
    }
};

template <bool H, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_capsule(DeviceScene S, NearestArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    listed_query<SegmentShape, H, COUNT>(S, Q, lds_stack);
}

} // namespace rtk

