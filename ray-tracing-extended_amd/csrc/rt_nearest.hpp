// rt_nearest.hpp — K-nearest point queries: EVERY surface within R of a point the caller supplies, nearest first, and how many there are
// (include/rt.h "K-nearest queries": options "closest_k" / "closest_all" of rt_closest_points): Unity's Physics.OverlapSphere beside
// ClosestPoint.  It is to k_closest what k_multihit is to k_ray_query: the same candidates, keys and records, a list instead of one winner.
//
// Definition (tests/nearest_oracle.c restates it as a brute-force loop and a sort): the closest-point queries' candidates and keys; a
// candidate counts when k < R * R; records 0 .. min(total, K) - 1 are the first of them in ascending (k, kind, uploaded index), the rest
// the miss record; _reserved[0] of all K records is min(total, K), or with closest_all the number of ALL candidates below R * R.
//
// k_closest's launch, walk and pieces (point_query, sphere_key, closest_node_step, closest_on_triangle, kCullSlack, kCullFloor, the two
// record writers, add_wave_counts: rt_closest.hpp) with k_multihit's list (HitList, rt_multihit.hpp: eight (key, id) pairs in
// registers, indexed at compile time only).  The kernels stay two for their registers: 49 VGPRs there, 64 here.  A sphere's id is s << 1, a triangle's
// kTriBit | ti << 1 with ti in BVH order: as unsigned numbers a sphere comes before a triangle, and between two triangles at one key
// HitList::insert compares the UPLOADED indices through order[].
//
// Pruning.  kb = R * R while slot K - 1 is empty or when closest_all is set, else the key in slot K - 1.  A child is skipped only when
// lb2 > max(kb * kCullSlack, kCullFloor): DESIGN.md "K-nearest queries" derives that no candidate whose key is <= the K-th lies in a
// skipped node.  A candidate enters the list when k <= the K-th key: equality passes, because a lower (kind, index) evicts the K-th.
// (With closest_all a candidate above the K-th key is counted and not inserted: it would only pass through slots K .. 7.)
#pragma once
#include "rt_closest.hpp"
#include "rt_multihit.hpp"

namespace rtk {

struct NearestArgs : ClosestArgs {      // (k_closest's fields first, in their order: out, counters)
    int k;                      // K, 1..8; out is [n*K*4] rt_closest, point-major
    int count_all;              // 1: the count is every candidate below R * R, and no pruning by the K-th key
};

template <bool H, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_nearest(DeviceScene S, NearestArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    const bool present = i < (unsigned)Q.n;
    if (!COUNT && !present) return;                                     // (the counting build keeps every lane for the wave's sums)
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const float INF = __builtin_inff();
    const PointQuery q = point_query(Q.in, i, present);
    const v3 p = q.p;
    const int K = Q.k;
    const bool count_all = Q.count_all != 0;
    const float r2 = q.R * q.R;
    HitList L;
    float kth = INF;                                    // key of slot K - 1: +inf until K candidates are in
    int total = 0;                                      // candidates below R * R (complete only when count_all)
    uint32_t n_nodes = 0, n_prims = 0;

    // (a macro: a lambda that captures the list by reference kept it in scratch, rt_multihit.hpp)
#define RT_OFFER(KEY, ID) { if ((KEY) < r2) { ++total; if ((KEY) <= kth) { L.insert((KEY), (ID), Q.order); kth = L.kth(K); } } }

    if (q.searched) {
        for (int s = 0; s < S.ns; ++s) {
            const float k = sphere_key(p, S.sph_geom[s]);
            if (COUNT) ++n_prims;
            RT_OFFER(k, (uint32_t)s << 1)
        }
        if (S.nn > 0) {
            const float4* nodes = H ? S.nodes_h : S.nodes;
            RT_WALK_NODE(stk, 0u)                                       // from the root
                if (COUNT) ++n_nodes;
                float l0, l1, l2, l3;
                uint32_t c0, c1, c2, c3;
                const float kb = count_all ? r2 : __builtin_fminf(r2, kth);     // (every key in the list is below r2)
                closest_node_step<H>(nodes, node, p, __builtin_fmaxf(kb * kCullSlack, kCullFloor), l0, l1, l2, l3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, c0 != kNone, c1 != kNone, c2 != kNone, c3 != kNone)
                float k, u, v;
                closest_on_triangle(p, tri_A, tri_AB, tri_AC, k, u, v);
                if (COUNT) ++n_prims;
                RT_OFFER(k, kTriBit | (ti << 1))
            RT_WALK_END(false)
        }
    }
#undef RT_OFFER

    // ---- the records: a winning triangle's test again for its (u, v) (the same operations, the same bits), then k_closest's record
    if (present) {
        const int count = count_all ? total : L.filled(K);
        float4* out = Q.out + 4 * ((size_t)i * (size_t)K);
        for (int j = 0; j < K; ++j) {
            float key; uint32_t id;
            L.pop_front(key, id);
            HitRecord rec;
            if (id == kNone) rec.miss(count);
            else if (id & kTriBit) {
                const uint32_t ti = (id & ~kTriBit) >> 1;
                float4 g0, g1, g2;
                load_tri(S.tri_geo, ti, g0, g1, g2);
                float k_again, u, v;
                closest_on_triangle(p, rtm::mk(g0.x, g0.y, g0.z), rtm::mk(g0.w, g1.x, g1.y), rtm::mk(g1.z, g1.w, g2.x), k_again, u, v);
                rec = closest_triangle_record(S, Q, p, ti, u, v, key, count);
            } else rec = closest_sphere_record(S, p, id >> 1, count);
            rec.store(out + 4 * (size_t)j);
        }
    }
    if (COUNT) add_wave_counts(Q.counters, n_nodes, n_prims);
}

} // namespace rtk
