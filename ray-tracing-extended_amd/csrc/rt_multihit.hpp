// rt_multihit.hpp — multi-hit ray queries: the first K surfaces along a ray the caller supplies, nearest first (include/rt.h rt_multihit,
// rt_trace_hits): Unity's Physics.RaycastAll beside closest hit and any hit.  Geometry only: intersectMode is the one rt_params field read.
//
// Definition (include/rt.h "multi-hit ray queries"; tests/hits_oracle.c restates it as a brute-force loop and a sort): every sphere and
// every triangle a chunk addresses is a candidate; RaySphere's entry root and RayTriangle's front hit count in either mode, the exit
// root and the back hit (det <= -1e-6f) in RT_HITS_BOTH as well; a hit counts when dst < tMax; the answer is the first K in ascending
// (dst, kind, uploaded index, side) — whatever the tree, the builder, the leaf size or the visiting order.
//
// k_ray_query's launch: one ray per lane, 256-thread blocks, one launch per slice, lane_stack's LDS stack with the global overflow,
// the per-lane walk (rt_kernels.hpp).  What is new is the per-lane list: eight (dst, id) pairs in registers, sorted, indexed at compile time
// only (K is a run-time value, but a run-time-indexed private array would live in scratch).  An accepted candidate is carried through
// the eight slots by compare-and-exchange, so slots 0 .. K-1 always hold the K smallest keys seen; slots K .. 7 hold whatever fell out
// of them and are never read.  Only keys are kept: the epilogue runs the primitive test again on the <= K winners (it is deterministic:
// the same bits) and writes the record with k_ray_query's expressions.
//
// Pruning.  bound = tMax while slot K-1 is empty or when countAll is set, else min(tMax, dst of slot K-1).  node_step keeps a child
// whose entry distance is <= bound (tn <= tf with tf clamped to the bound: equality passes), and a leaf candidate is dropped only when
// dst > dst of slot K-1: at equality the key decides, because a lower (kind, index, side) evicts the K-th.  dst < tMax stays strict.
#pragma once
#include "rt_query.hpp"

namespace rtk {

static_assert(sizeof(rt_multihit) == 64 && sizeof(rt_hits_params) == 32 && RT_HITS_MAX == 8, "a record is four float4 stores, the list has eight slots");

struct MultihitArgs : QueryHead {
    float4* out;                // [n*K*4]  rt_multihit, ray-major
    int max_hits;               // K, 1..8
    int count_all;              // 1: hitCount = every accepted hit below tMax, and no pruning by the K-th distance
};

// A list entry's id: a sphere is (index << 1) | exit, a triangle kTriBit | (BVH-order index << 1) | back; kNone = an empty slot (its
// dst is +inf).  As unsigned numbers the ids order sphere before triangle and front before back; between two triangles the UPLOADED
// index decides, read through `order` where it matters: at equal dst only.  (A triangle is hit from one side only, so the side bit
// never has to break a tie between triangles; a tangent sphere's two roots do tie, entry first.)
#define RT_HL_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
struct HitList {
#define RT_X(J) float d##J = __builtin_inff(); uint32_t i##J = kNone;
    RT_HL_SLOTS(RT_X)
#undef RT_X
    // dst of slot K - 1: +inf until K hits are in.  (The slots go to the select chain BY VALUE: written on the members, the chain of
    // selects over loads became one load at a selected address before this function was inlined, and the list went to scratch.)
    static __device__ __forceinline__ float pick(int K, float e0, float e1, float e2, float e3, float e4, float e5, float e6, float e7)
    {
        float b = e7;
        b = K <= 7 ? e6 : b; b = K <= 6 ? e5 : b; b = K <= 5 ? e4 : b; b = K <= 4 ? e3 : b;
        b = K <= 3 ? e2 : b; b = K <= 2 ? e1 : b; b = K <= 1 ? e0 : b;
        return b;
    }
    __device__ __forceinline__ float kth(int K) const { return pick(K, d0, d1, d2, d3, d4, d5, d6, d7); }
    // the candidate goes down the list: it takes the first slot whose key is larger and carries that slot's entry on.
    // INF_KEYS: the caller may offer a key of +inf (k_overlap: no radius bounds its keys), which ties with an EMPTY slot (+inf, kNone);
    // kNone has kTriBit set, so the tie read must be kept away from it — order[kNone >> 1] lies far outside the array.  The other
    // kernels offer finite keys only (dst < tMax, k < R * R) and keep the test they had.
    template <bool INF_KEYS = false>
    __device__ __forceinline__ void insert(float cd, uint32_t ci, const uint32_t* __restrict__ order)
    {
#define RT_X(J)                                                                                                          \
        {                                                                                                                \
            uint32_t ka_ = ci, kb_ = i##J;                                                                               \
            if (cd == d##J && ci != kNone && (!INF_KEYS || i##J != kNone) && (ci & i##J & kTriBit)) {   /* two triangles at one dst: rare */ \
                ka_ = order[(ci & ~kTriBit) >> 1]; kb_ = order[(i##J & ~kTriBit) >> 1];                                  \
            }                                                                                                            \
            const bool lt_ = cd < d##J || (cd == d##J && ka_ < kb_);                                                     \
            const float nd_ = lt_ ? cd : d##J, nc_ = lt_ ? d##J : cd;                                                    \
            const uint32_t ni_ = lt_ ? ci : i##J, nj_ = lt_ ? i##J : ci;                                                 \
            d##J = nd_; cd = nc_; i##J = ni_; ci = nj_;                                                                  \
        }
        RT_HL_SLOTS(RT_X)
#undef RT_X
    }
    // how many of slots 0 .. K-1 are in use
    __device__ __forceinline__ int filled(int K) const
    {
        int c = 0;
#define RT_X(J) c += (J < K && i##J != kNone) ? 1 : 0;
        RT_HL_SLOTS(RT_X)
#undef RT_X
        return c;
    }
    // slot 0 out, the others one slot down
    __device__ __forceinline__ void pop_front(float& d, uint32_t& id)
    {
        d = d0; id = i0;
        d0 = d1; d1 = d2; d2 = d3; d3 = d4; d4 = d5; d5 = d6; d6 = d7; d7 = __builtin_inff();
        i0 = i1; i1 = i2; i2 = i3; i3 = i4; i4 = i5; i5 = i6; i6 = i7; i7 = kNone;
    }
};
#undef RT_HL_SLOTS

// RayTriangle with both faces: +1 when RayTriangle accepts (front), -1 (BOTH only) when the same dst, u, v, w pass with det <= -1e-6f,
// else 0.  The front-only form IS ray_triangle.  inv must be the correctly rounded 1.0f / det on both sides: rcp_mid is verified for
// positive arguments, so it is taken of |det| and given det's sign (rounding to nearest is symmetric: 1 / -x = -(1 / x)); for a positive
// det these are ray_triangle's own operations.
template <bool BOTH>
__device__ __forceinline__ int ray_triangle_sided(v3 o, v3 d, v3 A, v3 eAB, v3 eAC, v3 n, float& dst, float& u, float& v)
{
    if constexpr (!BOTH) {
        return ray_triangle(o, d, A, eAB, eAC, n, dst, u, v) ? 1 : 0;
    } else {
        const v3 ao = o - A;
        const v3 dao = rtm::cross(ao, d);
        const float det = -rtm::dot(d, n);
        const float ad = __builtin_fabsf(det);
        float inv = rtm::rcp_mid(ad);
        if (ad > 0x1p100f) { RT_COLD_PATH(); inv = 1.0f / ad; }
        inv = __builtin_copysignf(inv, det);
        dst = rtm::dot(ao, n) * inv;
        u = rtm::dot(eAC, dao) * inv;
        v = -rtm::dot(eAB, dao) * inv;
        const float w = 1.0f - u - v;
        const bool inside = dst >= 0.0f && u >= 0.0f && v >= 0.0f && w >= 0.0f;
        return !inside ? 0 : det >= 1e-6f ? 1 : det <= -1e-6f ? -1 : 0;
    }
}

template <bool H, bool BOTH>
__global__ __launch_bounds__(kBlock) void k_multihit(DeviceScene S, MultihitArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float4 r0 = Q.in[2 * (size_t)i], r1 = Q.in[2 * (size_t)i + 1];
    const v3 o = rtm::mk(r0.x, r0.y, r0.z), d = rtm::mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w;
    const int K = Q.max_hits;
    const bool count_all = Q.count_all != 0;
    const float INF = __builtin_inff();
    HitList L;
    float kth = INF;                                    // dst of slot K - 1
    int total = 0;                                      // accepted hits below tMax (complete only when count_all)

    // an accepted candidate with dst < tMax that could still enter the list, or that a counting call counts
    // (a macro: a lambda that captures the list by reference kept it in scratch)
#define RT_OFFER(DST, ID) { ++total; if ((DST) <= kth) { L.insert((DST), (ID), Q.order); kth = L.kth(K); } }

    if (t_max > 0.0f) {                                 // tMax <= 0 or NaN: nothing is traced
        const float a = rtm::dot(d, d);
        const SphereA sa = sphere_a(a);
        for (int s = 0; s < S.ns; ++s) {
            const float4 sp = S.sph_geom[s];
            // RaySphere's b, c, disc; its root, and the other one from the same numbers
            const v3 oc = o - rtm::mk(sp.x, sp.y, sp.z);
            const float b = 2.0f * rtm::dot(oc, d);
            const float c = rtm::dot(oc, oc) - sp.w * sp.w;
            const float disc = b * b - 4.0f * sa.a * c;
            if (disc >= 0.0f) {
                const float sq = rtm::sqrt_(disc);
                const float t_in = sphere_quotient(sa, -b - sq);
                if (t_in >= 0.0f && t_in < t_max) RT_OFFER(t_in, (uint32_t)s << 1)
                if (BOTH) {
                    const float t_out = sphere_quotient(sa, -b + sq);
                    if (t_out >= 0.0f && t_out < t_max) RT_OFFER(t_out, ((uint32_t)s << 1) | 1u)
                }
            }
        }
        if (S.nn > 0 && ray_traceable(o, d, a)) {
            const RaySlabT<H> slab = make_slab<H>(o, d);
            RT_WALK_NODE(stk, 0u)                                       // from the root
                float t0, t1, t2, t3;
                uint32_t c0, c1, c2, c3;
                const float bound = count_all ? t_max : __builtin_fminf(t_max, kth);
                node_step<H>(H ? S.nodes_h : S.nodes, node, slab, bound, false, t0, t1, t2, t3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, t0 < INF, t1 < INF, t2 < INF, t3 < INF)
                float dst, u, v;
                const int side = ray_triangle_sided<BOTH>(o, d, tri_A, tri_AB, tri_AC, tri_n, dst, u, v);
                if (side != 0 && dst < t_max && (count_all || dst <= kth)) {
                    // the chunk filter's verdict is carried in dst, a float (rt_kernels.hpp, the per-lane walk)
                    if (Q.intersect_mode == RT_INTERSECT_FLAT_CHUNKS && !chunk_passes(S, ti, o, slab.inv)) dst = INF;
                    if (dst < INF) RT_OFFER(dst, kTriBit | (ti << 1) | (side < 0 ? 1u : 0u))
                }
            RT_WALK_END(false)
        }
    }
#undef RT_OFFER

    // ---- the records: the winners' tests again (their u, v), then k_ray_query's record with side and count
    const int hit_count = count_all ? total : L.filled(K);
    float4* out = Q.out + 4 * ((size_t)i * (size_t)K);
    for (int j = 0; j < K; ++j) {
        float dst; uint32_t id;
        L.pop_front(dst, id);
        HitRecord R;
        if (id == kNone) R.miss(hit_count);
        else {
            const v3 hitPoint = o + d * dst;
            const int side = (id & 1u) ? -1 : 1;
            v3 normal; const float4* mat;
            Hit h; h.t = dst; h.u = 0.f; h.v = 0.f;
            if (id & kTriBit) {
                const uint32_t ti = (id & ~kTriBit) >> 1;
                float4 g0, g1, g2;
                load_tri(S.tri_geo, ti, g0, g1, g2);
                float t_again;
                ray_triangle_sided<BOTH>(o, d, rtm::mk(g0.x, g0.y, g0.z), rtm::mk(g0.w, g1.x, g1.y), rtm::mk(g1.z, g1.w, g2.x),
                                         rtm::mk(g2.y, g2.z, g2.w), t_again, h.u, h.v);
                h.id = kTriBit | ti;
                surface_of(S, h, hitPoint, normal, mat);
                R.triangle(S, Q, ti, normal, h.u, h.v, side, hit_count);
            } else {
                h.id = id >> 1;
                surface_of(S, h, hitPoint, normal, mat);
                R.sphere(h.id, normal, side, hit_count);
            }
            R.at(dst, hitPoint);
        }
        R.store(out + 4 * (size_t)j);
    }
}

} // namespace rtk
