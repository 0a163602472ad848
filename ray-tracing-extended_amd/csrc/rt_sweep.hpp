// rt_sweep.hpp — sphere casts: how far a ball of radius r travels along a ray the caller supplies before it touches something, and
// where it touches (include/rt.h "sphere casts"; option "sweep" = 1 turns rt_trace_rays / rt_occluded and their device and rt_multi
// forms into this query): Unity's Physics.SphereCast beside Raycast, Linecast, RaycastAll and ClosestPoint.  Geometry only: no rt_params
// field is read, intersectMode included.
//
// Definition (include/rt.h; tests/sweep_oracle.c restates it as a brute-force loop): the radius is the float whose bits are
// rt_ray._reserved.  A scene sphere is RaySphere with the radii added.  A triangle has seven features — two faces (RayTriangle, both
// sides, from an origin moved by r along the unit normal), three edges (the ray against a cylinder of radius r) and three vertices
// (RaySphere of radius r) — and a feature's time t counts only when the ball at o + d * t really touches the triangle:
// closest_on_triangle's key there is at most g * g, g = r * (1 + 2^-6).  The smallest (t, kind, uploaded index, feature) with t < tMax
// wins, whatever the tree, the builder, the leaf size or the visiting order.
//
// k_ray_query's launch: one ray per lane, 256-thread blocks, one launch per slice, lane_stack's LDS stack with the global overflow, the
// per-lane walk (rt_kernels.hpp).  The node step's formula is this file's own, on the boxes child_boxes reads and with sort_children
// (rt_kernels.hpp, as closest_node_step): the slab test of boxes moved outwards by r * (1 + 2^-5) (at least
// 2^-60; +inf when g * g overflows), written as (plane - o) * (1 / d) so that a zero direction component gives -inf / +inf by the side of
// the plane the origin lies on, not a NaN.  DESIGN.md "Sphere casts" derives that no accepted candidate lies in a child that is skipped.
// A child is kept when its entry distance is <= min(tMax, best t): equality passes, a tie can still win on its index.
//
// Per triangle the seven times sit in seven named registers; the smallest that could still win is guarded first, and only if the guard
// refuses it the next one (a loop of at most seven trips around ONE copy of the region test).  Only (t, id, feature) is kept: the
// epilogue computes the winner's feature again (deterministic: the same bits) for hitPoint, u and v.
#pragma once
#include "rt_closest.hpp"
#include "rt_multihit.hpp"

namespace rtk {

struct SweepArgs : QueryHead {          // (intersect_mode is not read)
    float4* hits;               // [n*4]  rt_hit (closest contact)
    uint8_t* occluded;          // [n]    (any contact)
};

constexpr float kSweepGuard = 1.0f + 0x1p-6f;           // g = r * kSweepGuard: include/rt.h, tests/sweep_oracle.c
constexpr float kSweepInflate = 1.0f + 0x1p-5f;         // the boxes move outwards by r * kSweepInflate ...
constexpr float kSweepInflateFloor = 0x1p-60f;          // ... and never by less than this (a g * g that is denormal)

// The ray against the cylinder of radius r around the edge P + e * [0, 1]: the time of first contact, +inf when the feature does not
// answer.  s / ee is where on the edge (s and ee come back for the epilogue).
__device__ __forceinline__ float sweep_edge(v3 o, v3 d, float dd, float rr, v3 P, v3 e, float& s, float& ee)
{
    const v3 m = o - P;
    ee = rtm::dot(e, e);
    const float md = rtm::dot(m, e), nd = rtm::dot(d, e);
    const float qa = ee * dd - nd * nd;
    const float qb = ee * rtm::dot(m, d) - nd * md;
    const float qc = ee * (rtm::dot(m, m) - rr) - md * md;
    const float disc = qb * qb - qa * qc;
    const float t = (-qb - rtm::sqrt_(disc)) / qa;
    s = md + t * nd;
    return (qa > 0.0f && disc >= 0.0f && t >= 0.0f && s > 0.0f && s < ee) ? t : __builtin_inff();
}

// The four children of node `cur` for a ball: entry distances of the boxes moved outwards by infl, sorted ascending with their
// references; a child that is empty, or that the ray enters after `bound` or not at all, carries +inf.  sx, sy, sz: inv.x < 0, ...
template <bool H>
__device__ __forceinline__ void sweep_node_step(const float4* __restrict__ nodes, uint32_t cur, v3 o, v3 inv, bool sx, bool sy, bool sz,
                                                float infl, float bound, float& t0, float& t1, float& t2, float& t3,
                                                uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3)
{
    const float INF = __builtin_inff();
    const ChildBoxes b = child_boxes<H>(nodes, cur);
    c0 = b.ch.x; c1 = b.ch.y; c2 = b.ch.z; c3 = b.ch.w;
    // a NaN (0 * inf: the origin on a plane the ray runs along; inf - inf: an infinite inflation) is dropped by fmax / fmin: it passes
#define RT_SW(K, TK)                                                                                                     \
    {                                                                                                                    \
        const float ax_ = ((b.lox.K - infl) - o.x) * inv.x, bx_ = ((b.hix.K + infl) - o.x) * inv.x;                      \
        const float ay_ = ((b.loy.K - infl) - o.y) * inv.y, by_ = ((b.hiy.K + infl) - o.y) * inv.y;                      \
        const float az_ = ((b.loz.K - infl) - o.z) * inv.z, bz_ = ((b.hiz.K + infl) - o.z) * inv.z;                      \
        const float tn_ = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(sx ? bx_ : ax_, sy ? by_ : ay_), sz ? bz_ : az_), 0.0f);    \
        const float tf_ = __builtin_fminf(__builtin_fminf(__builtin_fminf(sx ? ax_ : bx_, sy ? ay_ : by_), sz ? az_ : bz_), bound);   \
        TK = (tn_ <= tf_) ? tn_ : INF;                                                                                   \
    }
    RT_SW(x, t0) RT_SW(y, t1) RT_SW(z, t2) RT_SW(w, t3)
#undef RT_SW
    // an empty slot holds a (+inf, -inf) box, which an infinite inflation turns into NaNs that pass: it is dropped by its reference
    if (c0 == kNone) t0 = INF;
    if (c1 == kNone) t1 = INF;
    if (c2 == kNone) t2 = INF;
    if (c3 == kNone) t3 = INF;
    // stack entries carry no distance, so the order in which the other three are popped is worth the two extra exchanges
    sort_children<false>(t0, t1, t2, t3, c0, c1, c2, c3);
}

template <bool ANY, bool H>
__global__ __launch_bounds__(kBlock) void k_sweep(DeviceScene S, SweepArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float4 r0 = Q.in[2 * (size_t)i], r1 = Q.in[2 * (size_t)i + 1];
    const v3 o = rtm::mk(r0.x, r0.y, r0.z), d = rtm::mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w, r = r1.w;                                 // (the radius: the bits of rt_ray._reserved)
    const float INF = __builtin_inff();
    // tMax <= 0 or NaN, r <= 0, NaN or infinite: a miss, nothing traced
    const bool traced = t_max > 0.0f && r > 0.0f && r <= 3.4028235e38f;
    float best_t = INF;                                                 // the best time so far
    uint32_t best = kNone;                                              // kNone | sphere index | kTriBit + triangle in BVH order
    int best_f = 0;                                                     // its feature code

    if (traced) {
        const float dd = rtm::dot(d, d), rr = r * r;
        const float g = r * kSweepGuard, g2 = g * g;
        const SphereA sa = sphere_a(dd);
        for (int s = 0; s < S.ns; ++s) {
            const float4 sp = S.sph_geom[s];
            float dst;
            // strict: the lower index keeps a tie
            if (ray_sphere(o, d, sa, rtm::mk(sp.x, sp.y, sp.z), sp.w + r, dst) && dst < t_max && dst < best_t) { best_t = dst; best = (uint32_t)s; }
        }
        if (S.nn > 0 && ray_traceable(o, d, dd)) {
            const v3 inv = rtm::mk(rtm::rcp_(d.x), rtm::rcp_(d.y), rtm::rcp_(d.z));
            const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;     // (of 1 / d, not of d: make_slab)
            const float infl = g2 <= 3.4028235e38f ? __builtin_fmaxf(r * kSweepInflate, kSweepInflateFloor) : INF;
            const float4* nodes = H ? S.nodes_h : S.nodes;
            RT_WALK_NODE(stk, (ANY && best_t < INF) ? kNone : 0u)       // from the root, unless a sphere answered an occlusion query
                float t0, t1, t2, t3;
                uint32_t c0, c1, c2, c3;
                sweep_node_step<H>(nodes, node, o, inv, sx, sy, sz, infl, __builtin_fminf(t_max, best_t), t0, t1, t2, t3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, t0 < INF, t1 < INF, t2 < INF, t3 < INF)
                // the seven features' times, +inf where a feature does not answer
                float f1, f2, f3, f4, f5, f6, f7, f8;
                {
                    const v3 sh = (tri_n * rtm::rcp_(rtm::sqrt_(rtm::dot(tri_n, tri_n)))) * r;
                    float u_, v_, s_, ee_;
                    f1 = INF; f2 = INF;
                    if (ray_triangle_sided<true>(o - sh, d, tri_A, tri_AB, tri_AC, tri_n, f6, u_, v_) == 1) f1 = f6;
                    if (ray_triangle_sided<true>(o + sh, d, tri_A, tri_AB, tri_AC, tri_n, f6, u_, v_) == -1) f2 = f6;
                    const v3 B = tri_A + tri_AB, C = tri_A + tri_AC;
                    f3 = sweep_edge(o, d, dd, rr, tri_A, tri_AB, s_, ee_);
                    f4 = sweep_edge(o, d, dd, rr, tri_A, tri_AC, s_, ee_);
                    f5 = sweep_edge(o, d, dd, rr, B, tri_AC - tri_AB, s_, ee_);
                    if (!ray_sphere(o, d, sa, tri_A, r, f6)) f6 = INF;
                    if (!ray_sphere(o, d, sa, B, r, f7)) f7 = INF;
                    if (!ray_sphere(o, d, sa, C, r, f8)) f8 = INF;
                }
                // only what could still win is worth a guard: t < tMax, and t <= the best so far (a tie can win on its index)
#define RT_X(F) F = (F < t_max && F <= best_t) ? F : INF;
                RT_X(f1) RT_X(f2) RT_X(f3) RT_X(f4) RT_X(f5) RT_X(f6) RT_X(f7) RT_X(f8)
#undef RT_X
#pragma nounroll
                for (;;) {
                    // the smallest (t, feature) left: strict comparisons in ascending code order keep the lower code at a tie
                    float tm = f1; int fm = 1;
#define RT_X(F, CODE) if (F < tm) { tm = F; fm = CODE; }
                    RT_X(f2, 2) RT_X(f3, 3) RT_X(f4, 4) RT_X(f5, 5) RT_X(f6, 6) RT_X(f7, 7) RT_X(f8, 8)
#undef RT_X
                    if (!(tm < INF)) break;
                    float k, u_, v_;
                    closest_on_triangle(o + d * tm, tri_A, tri_AB, tri_AC, k, u_, v_);
                    if (k <= g2) {                                      // the ball at tm touches the triangle: the candidate counts
                        bool take = tm < best_t;
                        // equal t: a sphere keeps the tie; between triangles the lower uploaded index wins
                        if (!take && best != kNone && (best & kTriBit)) take = Q.order[ti] < Q.order[best & ~kTriBit];
                        if (take) { best_t = tm; best = kTriBit | ti; best_f = fm; }
                        break;
                    }
#define RT_X(F, CODE) F = fm == CODE ? INF : F;
                    RT_X(f1, 1) RT_X(f2, 2) RT_X(f3, 3) RT_X(f4, 4) RT_X(f5, 5) RT_X(f6, 6) RT_X(f7, 7) RT_X(f8, 8)
#undef RT_X
                }
            RT_WALK_END(ANY && best_t < INF)                            // occlusion: the first accepted candidate ends the query
        }
    }

    if (ANY) {
        Q.occluded[i] = best_t < INF ? 1 : 0;
        return;
    }
    HitRecord rec;
    if (best == kNone) rec.miss(0);
    else {
        const v3 centre = o + d * best_t;                               // the ball's centre at the contact
        v3 point;
        if (best & kTriBit) {
            // the winner's feature again: the same operations as in the search, the same bits
            const uint32_t ti = best & ~kTriBit;
            float4 g0, g1, g2_;
            load_tri(S.tri_geo, ti, g0, g1, g2_);
            const v3 A = rtm::mk(g0.x, g0.y, g0.z), AB = rtm::mk(g0.w, g1.x, g1.y), AC = rtm::mk(g1.z, g1.w, g2_.x), n = rtm::mk(g2_.y, g2_.z, g2_.w);
            const v3 B = A + AB, C = A + AC;
            float u = 0.0f, v = 0.0f;
            if (best_f <= 2) {
                const v3 sh = (n * rtm::rcp_(rtm::sqrt_(rtm::dot(n, n)))) * r;
                const v3 o2 = best_f == 1 ? o - sh : o + sh;
                float t_again;
                ray_triangle_sided<true>(o2, d, A, AB, AC, n, t_again, u, v);
                point = o2 + d * t_again;
            } else if (best_f <= 5) {
                const v3 P = best_f == 5 ? B : A;
                const v3 e = best_f == 3 ? AB : best_f == 4 ? AC : AC - AB;
                float s, ee;
                sweep_edge(o, d, rtm::dot(d, d), r * r, P, e, s, ee);
                const float q = s / ee;
                point = P + e * q;
                if (best_f == 3) u = q;
                else if (best_f == 4) v = q;
                else { v = q; u = 1.0f - q; }
            } else {
                point = best_f == 6 ? A : best_f == 7 ? B : C;
                u = best_f == 7 ? 1.0f : 0.0f;
                v = best_f == 8 ? 1.0f : 0.0f;
            }
            rec.triangle(S, Q, ti, rtm::normalize(centre - point), u, v, best_f, 0);
        } else {
            const float4 sp = S.sph_geom[best];
            const v3 normal = rtm::normalize(centre - rtm::mk(sp.x, sp.y, sp.z));
            point = centre - normal * r;
            rec.sphere(best, normal, 0, 0);
        }
        rec.at(best_t, point);
    }
    rec.store(Q.hits + 4 * (size_t)i);
}

} // namespace rtk
