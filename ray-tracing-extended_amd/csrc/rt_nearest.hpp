// rt_nearest.hpp — K-nearest point queries: EVERY surface within R of a point the caller supplies, nearest first, and how many there are
// (include/rt.h "K-nearest queries": options "closest_k" / "closest_all" of rt_closest_points): Unity's Physics.OverlapSphere beside
// ClosestPoint.  It is to k_closest what k_multihit is to k_ray_query: the same candidates, keys and records, a list instead of one winner.
//
// Definition (tests/nearest_oracle.c restates it as a brute-force loop and a sort): the closest-point queries' candidates and keys; a
// candidate counts when k < R * R; records 0 .. min(total, K) - 1 are the first of them in ascending (k, kind, uploaded index), the rest
// the miss record; _reserved[0] of all K records is min(total, K), or with closest_all the number of ALL candidates below R * R.
//
// The listed-query frame (rt_listed.hpp) with k_closest's pieces (point_query, sphere_key, closest_node_step, closest_on_triangle, the
// two record writers: rt_closest.hpp).  The kernels stay two for their registers: 49 VGPRs there, 64 here.
//
// Pruning.  kb = R * R while slot K - 1 is empty or when closest_all is set, else the key in slot K - 1.  A child is skipped only when
// lb2 > max(kb * kCullSlack, kCullFloor): DESIGN.md "K-nearest queries" derives that no candidate whose key is <= the K-th lies in a
// skipped node.
#pragma once
#include "rt_listed.hpp"

namespace rtk {

struct PointShape : WithinReach<PointQuery> {
    static __device__ __forceinline__ PointShape load(const float4* __restrict__ in, unsigned int i, bool present)
    {
        return PointShape{ { point_query(in, i, present) } };
    }
    template <bool H>
    __device__ __forceinline__ void node_step(const float4* __restrict__ nodes, uint32_t cur, float thr, float& l0, float& l1, float& l2, float& l3,
                                              uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) const
    {
        closest_node_step<H>(nodes, cur, p, p, thr, l0, l1, l2, l3, c0, c1, c2, c3);
    }
    __device__ __forceinline__ bool sphere(float4 sp, float& k) const { k = sphere_key(p, sp); return true; }
    __device__ __forceinline__ bool triangle(v3 A, v3 AB, v3 AC, v3, float& k) const
    {
        float u, v;
        closest_on_triangle(p, A, AB, AC, k, u, v);
        return true;
    }
    // a listed triangle's test again for its (u, v), then k_closest's records
    __device__ __forceinline__ HitRecord triangle_record(const DeviceScene& S, const QueryHead& Q, uint32_t ti, v3 A, v3 AB, v3 AC, v3,
                                                         float key, int count) const
    {
        float k_again, u, v;
        closest_on_triangle(p, A, AB, AC, k_again, u, v);
        return closest_triangle_record(S, Q, p, ti, u, v, key, count);
    }
    __device__ __forceinline__ HitRecord sphere_record(const DeviceScene& S, uint32_t si, int count) const
    {
        return closest_sphere_record(S, p, si, count);
    }
};

template <bool H, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_nearest(DeviceScene S, NearestArgs Q)
{
    extern __shared__ uint32_t lds_stack[];
    listed_query<PointShape, H, COUNT>(S, Q, lds_stack);
}

} // namespace rtk
