// rt_listed.hpp — the listed-query frame: what k_nearest, k_overlap and k_capsule have in common.  Each is this frame plus a Shape.
//
// A listed query answers an input of rt_closest_points with the K best candidates, in ascending (key, kind, uploaded index), and their
// count: k_closest's launch, walk and record writers (rt_closest.hpp) with k_multihit's list (HitList, rt_multihit.hpp: eight (key, id)
// pairs in registers, indexed at compile time only).  A sphere's id is s << 1, a triangle's kTriBit | ti << 1 with ti in BVH order: as
// unsigned numbers a sphere comes before a triangle, and between two triangles at one key HitList::insert compares the UPLOADED indices
// through order[].  A candidate that counts enters the list when k <= the K-th key: equality passes, because a lower (kind, index)
// evicts the K-th.  (With closest_all a candidate above the K-th key is counted and not inserted: it would only pass through slots
// K .. 7.)  The list holds (key, id) only: the epilogue has the shape run a listed winner's test again for its coordinates (the same
// operations, the same bits).
//
// A Shape is what one family reads from an input and how it tests a candidate (PointShape rt_nearest.hpp, BoxShape rt_overlap.hpp,
// SegmentShape rt_capsule.hpp); the frame hands it values and references to scalars only:
//     static Shape load(in, i, present)        input i, and `searched`: false where the input has no candidate by its own values
//     kInfKeys                                 a counted key can be +inf (HitList::insert<true>)
//     admits(k)                                the key of a candidate that passed sphere() / triangle() counts
//     threshold(count_all, kth)                the largest squared lower bound of a node that is still visited
//     node_step<H>(nodes, node, thr, l0 .. l3, c0 .. c3)      closest_node_step's contract
//     sphere(sp, k), triangle(A, AB, AC, n, k)                the candidate's key; false: it cannot count, k is not read
//     sphere_record(S, si, count), triangle_record(S, Q, ti, A, AB, AC, n, key, count)     a listed winner's record
// The list is a local of the frame and goes to no Shape member: a lambda that captured it by reference kept it in scratch
// (rt_multihit.hpp), hence RT_OFFER is a macro.
#pragma once
#include "rt_closest.hpp"
#include "rt_multihit.hpp"

namespace rtk {

struct NearestArgs : ClosestArgs {      // (k_closest's fields first, in their order: out, counters)
    int k;                      // K, 1..8; out is [n*K*4] rt_closest, point-major
    int count_all;              // 1: the count is every candidate that counts, and no pruning by the K-th key
};

// The rule of the shapes with a reach R (Query has it as a member): a key counts below R * R, and kb = R * R while slot K - 1 is empty
// or when closest_all is set, else the key in slot K - 1 (every key in the list is below R * R)
template <class Query> struct WithinReach : Query {
    static constexpr bool kInfKeys = false;
    __device__ __forceinline__ bool admits(float k) const { return k < this->R * this->R; }
    __device__ __forceinline__ float threshold(bool count_all, float kth) const
    {
        const float r2 = this->R * this->R;
        return __builtin_fmaxf((count_all ? r2 : __builtin_fminf(r2, kth)) * kCullSlack, kCullFloor);
    }
};

template <class Shape, bool H, bool COUNT>
__device__ __forceinline__ void listed_query(const DeviceScene& S, const NearestArgs& Q, uint32_t* lds_stack)
{
    const unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    const bool present = i < (unsigned)Q.n;
    if (!COUNT && !present) return;                                     // (the counting build keeps every lane for the wave's sums)
    const TravStack stk = lane_stack(lds_stack, Q.stack_cap, Q.gstack, Q.gstack_stride);
    const Shape q = Shape::load(Q.in, i, present);
    const int K = Q.k;
    const bool count_all = Q.count_all != 0;
    HitList L;
    float kth = __builtin_inff();                       // key of slot K - 1: +inf until K candidates are in
    int total = 0;                                      // candidates that count (complete only when count_all)
    uint32_t n_nodes = 0, n_prims = 0;

#define RT_OFFER(KEY, ID) { if (q.admits(KEY)) { ++total; if ((KEY) <= kth) { L.insert<Shape::kInfKeys>((KEY), (ID), Q.order); kth = L.kth(K); } } }

    if (q.searched) {
        for (int s = 0; s < S.ns; ++s) {
            float k;
            const bool counts = q.sphere(S.sph_geom[s], k);
            if (COUNT) ++n_prims;
            if (counts) RT_OFFER(k, (uint32_t)s << 1)
        }
        if (S.nn > 0) {
            const float4* nodes = H ? S.nodes_h : S.nodes;
            RT_WALK_NODE(stk, 0u)                                       // from the root
                if (COUNT) ++n_nodes;
                float l0, l1, l2, l3;
                uint32_t c0, c1, c2, c3;
                q.template node_step<H>(nodes, node, q.threshold(count_all, kth), l0, l1, l2, l3, c0, c1, c2, c3);
            RT_WALK_TRIANGLE(S.tri_geo, c0 != kNone, c1 != kNone, c2 != kNone, c3 != kNone)
                float k;
                const bool counts = q.triangle(tri_A, tri_AB, tri_AC, tri_n, k);
                if (COUNT) ++n_prims;
                if (counts) RT_OFFER(k, kTriBit | (ti << 1))
            RT_WALK_END(false)
        }
    }
#undef RT_OFFER

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
                rec = q.triangle_record(S, Q, ti, rtm::mk(g0.x, g0.y, g0.z), rtm::mk(g0.w, g1.x, g1.y), rtm::mk(g1.z, g1.w, g2.x),
                                        rtm::mk(g2.y, g2.z, g2.w), key, count);
            } else rec = q.sphere_record(S, id >> 1, count);
            rec.store(out + 4 * (size_t)j);
        }
    }
    if (COUNT) add_wave_counts(Q.counters, n_nodes, n_prims);
}

} // namespace rtk
