// rt_visibility.hpp — visibility gathers: how much of the hemisphere or sphere around a POINT is open, in which direction, and how far
// away the surfaces are (include/rt.h rt_visibility).  Ambient occlusion and bent normals of a lightmap texel, the sky visibility and
// visibility SH9 of a probe, the distance moments that place probes.  Geometry only: no rt_params field but intersectMode is read and
// nothing is shaded.
//
// Definition (include/rt.h "visibility gathers"; tests/query_oracle.c runs the oracle's own random_direction() and
// calculate_ray_collision() for it):
//   direction     rt_gather's, bit for bit (gather_direction of rt_gather.hpp is CALLED, not copied: using it here changes nothing in
//                 k_gather): key (firstIndex + i, seed), counter (block, s), blocks 0xFFFFFFFE / 0xFFFFFFFF.  RT_VIS_COSINE and
//                 RT_VIS_DISTANCE: d = normalize(n + R); RT_VIS_SH9: d = R
//   cast          modes 0, 1: v = 1 unless rt_occluded's rule finds a hit with dst < tMax (any_hit); mode 2: rt_trace_rays' closest hit
//                 bounded by tMax (closest_hit), r = its dst or tMax, hit = 1 / 0
//   channels      mode 0: (v ? d : 0, v); mode 1: (v ? Y_k(d) : 0 for k = 0..8, v); mode 2: (r, r * r, hit) — selects, never products
//   sum           the Philox mode's tree over the N samples per channel, root / N; mode 1: coefficients * 4 pi after the division.
//                 tMax <= 0 or NaN: zeros, no draw, no cast
//
// The launch, the lane layout (an item is a point) and the estimator's tree are the sample-lane frame's (rt_sampled.hpp); the next
// sample's ray is made as k_gather makes it, written out here.  The loop is flatter than k_gather's: a sample is ONE cast, so a trip is one traversal site
// (any_hit or closest_hit) and the sums.
#pragma once
#include "rt_gather.hpp"

namespace rtk {

struct VisibilityArgs : SampledHead {               // in: the points, (normal, -) second; out: [n] (COSINE, DISTANCE) or [n*3] (SH9)
    int sample_lanes_log2;      // log2 S
    int intersect_mode;         // as QueryArgs
    int stack_cap, full_sort;   // as QueryArgs
    uint32_t* gstack; unsigned int gstack_stride;
};
static_assert(sizeof(SampledHead) == 32 && sizeof(VisibilityArgs) == 64, "a kernel argument moved");

template <int MODE, bool H>
__global__ __launch_bounds__(kBlock) void k_visibility(DeviceScene S, VisibilityArgs A)
{
    extern __shared__ uint32_t lds_stack[];
    constexpr int NC = MODE == RT_VIS_SH9 ? 10 : MODE == RT_VIS_DISTANCE ? 3 : 4;       // channels per point
    constexpr int DIR = MODE == RT_VIS_SH9 ? RT_GATHER_SH9 : RT_GATHER_COSINE;         // the draw rt_gather makes for these directions
    const SampleLane L = sample_lane(A);
    if (L.idle_wave) return;
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);
    const float INF = __builtin_inff();

    v3 o = rtm::mk(0.f, 0.f, 0.f), d = o;
    float t_bound = 0.0f;
    if (L.present) {
        const float4 r0 = A.in[2 * (size_t)L.item];
        o = rtm::mk(r0.x, r0.y, r0.z);
        t_bound = r0.w;
    }
    const bool traced = t_bound > 0.0f;                                 // tMax <= 0 or NaN: zeros, nothing drawn or traced
    const uint32_t key = A.first_index + L.item;                        // first Philox key word: the item's index in the call's stream

    float total[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) total[k] = 0.0f;
    int sample = L.sub;
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0;
    bool alive = L.present && traced && sample < A.samples;
    if (alive) {
        const float4 r1 = A.in[2 * (size_t)L.item + 1];
        d = gather_direction<DIR>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
    }

    while (alive) {
        if constexpr (MODE == RT_VIS_DISTANCE) {
            const Hit h = closest_hit<false, H>(S, A.intersect_mode, full_sort, o, d, stk, cnt, t_bound);
            const float r = h.id != kNone ? h.t : t_bound;
            total[0] = total[0] + r;
            total[1] = total[1] + r * r;
            total[2] = total[2] + (h.id != kNone ? 1.0f : 0.0f);
        } else {
            const float hit_t = any_hit<H>(S, A.intersect_mode, o, d, t_bound, stk);
            const bool open = !(hit_t < INF);                           // (compared after the merge: the per-lane walk records why)
            if constexpr (MODE == RT_VIS_SH9) {
                float Y[9];
                sh9_basis(d, Y);
#pragma unroll
                for (int k = 0; k < 9; ++k) total[k] = total[k] + (open ? Y[k] : 0.0f);
                total[9] = total[9] + (open ? 1.0f : 0.0f);
            } else {
                total[0] = total[0] + (open ? d.x : 0.0f);
                total[1] = total[1] + (open ? d.y : 0.0f);
                total[2] = total[2] + (open ? d.z : 0.0f);
                total[3] = total[3] + (open ? 1.0f : 0.0f);
            }
        }
        sample += L.nsub;
        if (sample >= A.samples) alive = false;
        else {
            // the next sample starts at the point again, along a direction of its own
            const float4 r0 = A.in[2 * (size_t)L.item], r1 = A.in[2 * (size_t)L.item + 1];
            o = rtm::mk(r0.x, r0.y, r0.z);
            t_bound = r0.w;
            d = gather_direction<DIR>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
        }
    }

    tree_sum<NC>(total, L.nsub);
    if (L.stores()) {
        const float nf = (float)A.samples;
        if constexpr (MODE == RT_VIS_SH9) {
            float4* out = A.out + 3 * (size_t)L.item;
            float c[12];
#pragma unroll
            for (int k = 0; k < 9; ++k) c[k] = (total[k] / nf) * 12.566371f;
            c[9] = total[9] / nf; c[10] = 0.0f; c[11] = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                out[k] = traced ? make_float4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (MODE == RT_VIS_DISTANCE) {
            A.out[L.item] = traced ? make_float4(total[0] / nf, total[1] / nf, total[2] / nf, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            A.out[L.item] = traced ? make_float4(total[0] / nf, total[1] / nf, total[2] / nf, total[3] / nf) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

} // namespace rtk
