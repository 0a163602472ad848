// rt_sweep_all.hpp — sphere-cast-all: the first K surfaces a ball of radius r touches while it travels along a ray the caller supplies, in
// order (include/rt.h "sphere-cast-all"; option "hits_sweep" = 1 turns rt_trace_hits and its device and rt_multi forms into this query):
// Unity's Physics.SphereCastAll beside SphereCast and RaycastAll.  Geometry only: intersectMode is not read, the test is two-sided.
//
// Definition (include/rt.h; tests/sweep_all_oracle.c restates it as a brute-force loop and a sort): a primitive is one candidate at most,
// and it is what "sphere casts" defines for that primitive alone — a scene sphere by RaySphere with the radii added, a triangle by the
// smallest (t, code) among its eight feature codes with t < tMax whose ball really touches it (the guard).  The answer is the first K in
// ascending (t, kind, uploaded index), whatever the tree, the builder, the leaf size or the visiting order.
//
// Both halves are included, not copied: k_sweep's launch shape, sweep_edge and sweep_node_step (rt_sweep.hpp), and k_multihit's
// register-resident HitList with its offer macro (rt_multihit.hpp).  An id is sphere << 1, or kTriBit | BVH index << 1: the low bit,
// k_multihit's side bit, is always 0, so HitList::insert and its tie read through Q.order need no change.  The per-triangle steps —
// sweep_times, sweep_first_touch, sweep_contact — restate k_sweep's inline text as value-taking functions, because this kernel runs them
// twice (search and epilogue).  k_sweep does not call them, for a measured reason: with sweep_candidate and sweep_contact in place of its
// own text (7 to 14 instructions more, 85 -> 82 VGPRs) every sphere_cast and sphere_check row ran 0.7 % to 1.6 % slower than the parent's
// slowest run, in two sessions, and its own text inside the same library did not (profiles/ray_list_frame_timing.txt).  The same file
// holds what one frame for this kernel and k_multihit cost k_multihit's front-face rows (+0.4 % to +1.0 %): both keep their text.
//
// Pruning (DESIGN.md "Sphere-cast-all").  bound = tMax while slot K-1 is empty or when countAll is set, else min(tMax, t of slot K-1);
// sweep_node_step keeps a child whose entry distance is <= bound, and a triangle's features with t > the K-th t are dropped before the
// guard: that cannot change the triangle's candidate when the candidate is <= the K-th t (the smaller features fail the guard either way),
// and a candidate beyond the K-th t is not wanted.  A counting call drops nothing but t >= tMax.
#pragma once
#include "rt_sweep.hpp"

namespace rtk {

// The eight feature codes' times of one triangle (1, 2: the faces from the front and from behind; 3..5: edges AB, AC, BC; 6..8: vertices
// A, B, C), +inf where a feature does not answer
__device__ __forceinline__ void sweep_times(v3 o, v3 d, float dd, float rr, float r, const SphereA& sa, v3 A, v3 AB, v3 AC, v3 n,
                                            float& f1, float& f2, float& f3, float& f4, float& f5, float& f6, float& f7, float& f8)
{
    const float INF = __builtin_inff();
    const v3 sh = (n * rtm::rcp_(rtm::sqrt_(rtm::dot(n, n)))) * r;
    float u_, v_, s_, ee_;
    f1 = INF; f2 = INF;
    if (ray_triangle_sided<true>(o - sh, d, A, AB, AC, n, f6, u_, v_) == 1) f1 = f6;
    if (ray_triangle_sided<true>(o + sh, d, A, AB, AC, n, f6, u_, v_) == -1) f2 = f6;
    const v3 B = A + AB, C = A + AC;
    f3 = sweep_edge(o, d, dd, rr, A, AB, s_, ee_);
    f4 = sweep_edge(o, d, dd, rr, A, AC, s_, ee_);
    f5 = sweep_edge(o, d, dd, rr, B, AC - AB, s_, ee_);
    if (!ray_sphere(o, d, sa, A, r, f6)) f6 = INF;
    if (!ray_sphere(o, d, sa, B, r, f7)) f7 = INF;
    if (!ray_sphere(o, d, sa, C, r, f8)) f8 = INF;
}

// The smallest (t, code) among the times left finite at which the ball really touches the triangle (closest_on_triangle's key of the
// centre is at most g2): a loop of at most eight trips around ONE copy of the region test.  false: none passes.
__device__ __forceinline__ bool sweep_first_touch(v3 o, v3 d, float g2, v3 A, v3 AB, v3 AC, float f1, float f2, float f3, float f4, float f5,
                                                  float f6, float f7, float f8, float& tm, int& fm)
{
    const float INF = __builtin_inff();
#pragma nounroll
    for (;;) {
        // the smallest (t, feature) left: strict comparisons in ascending code order keep the lower code at a tie
        tm = f1; fm = 1;
#define RT_X(F, CODE) if (F < tm) { tm = F; fm = CODE; }
        RT_X(f2, 2) RT_X(f3, 3) RT_X(f4, 4) RT_X(f5, 5) RT_X(f6, 6) RT_X(f7, 7) RT_X(f8, 8)
#undef RT_X
        if (!(tm < INF)) return false;
        float k, u_, v_;
        closest_on_triangle(o + d * tm, A, AB, AC, k, u_, v_);
        if (k <= g2) return true;                           // the ball at tm touches the triangle: the candidate counts
#define RT_X(F, CODE) F = fm == CODE ? INF : F;
        RT_X(f1, 1) RT_X(f2, 2) RT_X(f3, 3) RT_X(f4, 4) RT_X(f5, 5) RT_X(f6, 6) RT_X(f7, 7) RT_X(f8, 8)
#undef RT_X
    }
}

// Where the ball at time t touches triangle (A, AB, AC, n) through feature f: the feature's test again (the same operations as in the
// search, the same bits) for the contact point and its (u, v)
__device__ __forceinline__ void sweep_contact(v3 o, v3 d, float r, v3 A, v3 AB, v3 AC, v3 n, int f, v3& point, float& u, float& v)
{
    const v3 B = A + AB, C = A + AC;
    u = 0.0f; v = 0.0f;
    if (f <= 2) {
        const v3 sh = (n * rtm::rcp_(rtm::sqrt_(rtm::dot(n, n)))) * r;
        const v3 o2 = f == 1 ? o - sh : o + sh;
        float t_again;
        ray_triangle_sided<true>(o2, d, A, AB, AC, n, t_again, u, v);
        point = o2 + d * t_again;
    } else if (f <= 5) {
        const v3 P = f == 5 ? B : A;
        const v3 e = f == 3 ? AB : f == 4 ? AC : AC - AB;
        float s, ee;
        sweep_edge(o, d, rtm::dot(d, d), r * r, P, e, s, ee);
        const float q = s / ee;
        point = P + e * q;
        if (f == 3) u = q;
        else if (f == 4) v = q;
        else { v = q; u = 1.0f - q; }
    } else {
        point = f == 6 ? A : f == 7 ? B : C;
        u = f == 7 ? 1.0f : 0.0f;
        v = f == 8 ? 1.0f : 0.0f;
    }
}

// A triangle's candidate: the smallest (t, code) with t < t_max and t <= limit that passes the guard.  false: none.
__device__ __forceinline__ bool sweep_candidate(v3 o, v3 d, float dd, float rr, float r, const SphereA& sa, float g2, v3 A, v3 AB, v3 AC, v3 n,
                                                float t_max, float limit, float& tm, int& fm)
{
    const float INF = __builtin_inff();
    float f1, f2, f3, f4, f5, f6, f7, f8;
    sweep_times(o, d, dd, rr, r, sa, A, AB, AC, n, f1, f2, f3, f4, f5, f6, f7, f8);
#define RT_X(F) F = (F < t_max && F <= limit) ? F : INF;
    RT_X(f1) RT_X(f2) RT_X(f3) RT_X(f4) RT_X(f5) RT_X(f6) RT_X(f7) RT_X(f8)
#undef RT_X
    return sweep_first_touch(o, d, g2, A, AB, AC, f1, f2, f3, f4, f5, f6, f7, f8, tm, fm);
}

template <bool H>
__global__ __launch_bounds__(kBlock) void k_sweep_all(DeviceScene S, MultihitArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float4 r0 = Q.in[2 * (size_t)i], r1 = Q.in[2 * (size_t)i + 1];
    const v3 o = rtm::mk(r0.x, r0.y, r0.z), d = rtm::mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w, r = r1.w;                                 // (the radius: the bits of rt_ray._reserved)
    const int K = Q.max_hits;
    const bool count_all = Q.count_all != 0;
    const float INF = __builtin_inff();
    // tMax <= 0 or NaN, r <= 0, NaN or infinite: K empty records, nothing traced
    const bool traced = t_max > 0.0f && r > 0.0f && r <= 3.4028235e38f;
    const float dd = rtm::dot(d, d), rr = r * r;
    const float g = r * kSweepGuard, g2 = g * g;
    const SphereA sa = sphere_a(dd);
    HitList L;
    float kth = INF;                                    // t of slot K - 1
    int total = 0;                                      // candidates below tMax (complete only when count_all)

    // (a macro, as in k_multihit: a lambda that captures the list by reference kept it in scratch)
#define RT_OFFER(T, ID) { ++total; if ((T) <= kth) { L.insert((T), (ID), Q.order); kth = L.kth(K); } }

    if (traced) {
        for (int s = 0; s < S.ns; ++s) {
            const float4 sp = S.sph_geom[s];
            float dst;
            if (ray_sphere(o, d, sa, rtm::mk(sp.x, sp.y, sp.z), sp.w + r, dst) && dst < t_max) RT_OFFER(dst, (uint32_t)s << 1)
        }
        if (S.nn > 0 && ray_traceable(o, d, dd)) {
            const v3 inv = rtm::mk(rtm::rcp_(d.x), rtm::rcp_(d.y), rtm::rcp_(d.z));
            const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;     // (of 1 / d, not of d: make_slab)
            const float infl = g2 <= 3.4028235e38f ? __builtin_fmaxf(r * kSweepInflate, kSweepInflateFloor) : INF;
            const float4* nodes = H ? S.nodes_h : S.nodes;
            RT_WALK_NODE(stk, 0u)                                       // from the root
                float t0, t1, t2, t3;
                uint32_t c0, c1, c2, c3;
                const float bound = count_all ? t_max : __builtin_fminf(t_max, kth);
                sweep_node_step<H>(nodes, node, o, inv, sx, sy, sz, infl, bound, t0, t1, t2, t3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, t0 < INF, t1 < INF, t2 < INF, t3 < INF)
                // the first feature that passes is the triangle's candidate; beyond the K-th t nothing is wanted unless the call counts
                float tm; int fm;
                if (sweep_candidate(o, d, dd, rr, r, sa, g2, tri_A, tri_AB, tri_AC, tri_n, t_max, count_all ? INF : kth, tm, fm))
                    RT_OFFER(tm, kTriBit | (ti << 1))
            RT_WALK_END(false)
        }
    }
#undef RT_OFFER

    // ---- the records: a triangle winner's feature again (deterministic: the same bits), then k_sweep's record with side, count and code
    const int hit_count = count_all ? total : L.filled(K);
    float4* out = Q.out + 4 * ((size_t)i * (size_t)K);
    for (int j = 0; j < K; ++j) {
        float t; uint32_t id;
        L.pop_front(t, id);
        HitRecord R;
        if (id == kNone) R.miss(hit_count);
        else {
            const v3 centre = o + d * t;                                // the ball's centre at the contact
            v3 point;
            if (id & kTriBit) {
                const uint32_t ti = (id & ~kTriBit) >> 1;
                float4 q0, q1, q2;
                load_tri(S.tri_geo, ti, q0, q1, q2);
                const v3 A = rtm::mk(q0.x, q0.y, q0.z), AB = rtm::mk(q0.w, q1.x, q1.y), AC = rtm::mk(q1.z, q1.w, q2.x), n = rtm::mk(q2.y, q2.z, q2.w);
                float tm, u, v; int fm;
                // (nothing later than t can be the candidate that t came from)
                sweep_candidate(o, d, dd, rr, r, sa, g2, A, AB, AC, n, t_max, t, tm, fm);
                sweep_contact(o, d, r, A, AB, AC, n, fm, point, u, v);
                // which side of the face the centre is on at the contact; 0 also for a NaN
                const float sd = rtm::dot(centre - point, rtm::cross(AB, AC));
                R.triangle(S, Q, ti, rtm::normalize(centre - point), u, v, sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0, hit_count);
                R.w3.w = __int_as_float(fm);                            // rt_multihit._reserved: the feature code
            } else {
                const uint32_t si = id >> 1;
                const float4 sp = S.sph_geom[si];
                const v3 normal = rtm::normalize(centre - rtm::mk(sp.x, sp.y, sp.z));
                point = centre - normal * r;
                R.sphere(si, normal, 1, hit_count);
            }
            R.at(t, point);
        }
        R.store(out + 4 * (size_t)j);
    }
}

} // namespace rtk
