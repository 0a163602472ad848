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
// k_gather's launch, lane layout and tree: a point's S = 16 / 4 / 1 sub-streams sit on S ADJACENT lanes (lane = point * S + sub-stream),
// lane k walks samples k, k + S, ..., four xor-exchanges per channel at lane distances 1, 2, 4, 8, every lane of the wave takes part,
// lanes without a point carry zeros, the sub-stream-0 lane stores.  The loop is flatter than k_gather's: a sample is ONE cast, so a
// trip is one traversal site (any_hit or closest_hit) and the sums.  The two lessons the other kernels record hold here: hit or miss
// crosses the traversal as a value (any_hit's hit_t, closest_hit's h.id), never as a bool; and the next sample's direction is drawn at
// the END of a trip, once before the loop, so every lane arrives at the traversal with its ray ready.  The point is read again from memory
// there: the normal does not live across the traversal.
#pragma once
#include "rt_gather.hpp"

namespace rtk {

struct VisibilityArgs {
    const float4* points;       // [n*2]  rt_ray: (origin, tMax) (normal, -)
    float4* out;                // [n] (COSINE, DISTANCE) or [n*3] (SH9)
    int n;
    int samples;                // N
    uint32_t seed;              // second key word
    uint32_t first_index;       // first key word of point 0 of this launch
    int sample_lanes_log2;      // log2 S
    int intersect_mode;         // as QueryArgs
    int stack_cap, full_sort;   // as QueryArgs
    uint32_t* gstack; unsigned int gstack_stride;
};

template <int MODE, bool H>
__global__ __launch_bounds__(kBlock) void k_visibility(DeviceScene S, VisibilityArgs A)
{
    extern __shared__ uint32_t lds_stack[];
    constexpr int NC = MODE == RT_VIS_SH9 ? 10 : MODE == RT_VIS_DISTANCE ? 3 : 4;       // channels per point
    constexpr int DIR = MODE == RT_VIS_SH9 ? RT_GATHER_SH9 : RT_GATHER_COSINE;         // the draw rt_gather makes for these directions
    const int sl = A.sample_lanes_log2, nsub = 1 << sl;
    const unsigned int g = blockIdx.x * kBlock + threadIdx.x;          // (the host keeps points-per-launch * S below 2^31)
    if ((g & ~63u) >> sl >= (unsigned)A.n) return;                      // (wave-uniform: no lane of this wave has a point)
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);
    const unsigned int point = g >> sl;
    const int sub = (int)(g & (unsigned)(nsub - 1));
    const bool present = point < (unsigned)A.n;
    const float INF = __builtin_inff();

    v3 o = rtm::mk(0.f, 0.f, 0.f), d = o;
    float t_bound = 0.0f;
    if (present) {
        const float4 r0 = A.points[2 * (size_t)point];
        o = rtm::mk(r0.x, r0.y, r0.z);
        t_bound = r0.w;
    }
    const bool traced = t_bound > 0.0f;                                 // tMax <= 0 or NaN: zeros, nothing drawn or traced
    const uint32_t key = A.first_index + point;

    // this lane's sub-stream: samples sub, sub + S, ... in increasing order, every channel summed from 0
    float total[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) total[k] = 0.0f;
    int sample = sub;
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0;
    bool alive = present && traced && sample < A.samples;
    if (alive) {
        const float4 r1 = A.points[2 * (size_t)point + 1];
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
                // the real SH basis of bands 0..2 on the drawn direction, every product its own rounding (include/rt.h)
                const float x = d.x, y = d.y, z = d.z;
                float Y[9];
                Y[0] = 0.28209479f;
                Y[1] = 0.48860251f * y;
                Y[2] = 0.48860251f * z;
                Y[3] = 0.48860251f * x;
                Y[4] = 1.09254843f * (x * y);
                Y[5] = 1.09254843f * (y * z);
                Y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
                Y[7] = 1.09254843f * (x * z);
                Y[8] = 0.54627421f * (x * x - y * y);
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
        sample += nsub;
        if (sample >= A.samples) alive = false;
        else {
            // the next sample starts at the point again, along a direction of its own
            const float4 r0 = A.points[2 * (size_t)point], r1 = A.points[2 * (size_t)point + 1];
            o = rtm::mk(r0.x, r0.y, r0.z);
            t_bound = r0.w;
            d = gather_direction<DIR>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
        }
    }

    // the estimator's tree: (k, k + 1) for even k, then (k, k + 2) for k = 0 mod 4, ...
    for (int off = 1; off < nsub; off <<= 1) {
#pragma unroll
        for (int k = 0; k < NC; ++k) total[k] = total[k] + __shfl_xor(total[k], off, 64);
    }
    if (present && sub == 0) {
        const float nf = (float)A.samples;
        if constexpr (MODE == RT_VIS_SH9) {
            float4* out = A.out + 3 * (size_t)point;
            float c[12];
#pragma unroll
            for (int k = 0; k < 9; ++k) c[k] = (total[k] / nf) * 12.566371f;
            c[9] = total[9] / nf; c[10] = 0.0f; c[11] = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                out[k] = traced ? make_float4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (MODE == RT_VIS_DISTANCE) {
            A.out[point] = traced ? make_float4(total[0] / nf, total[1] / nf, total[2] / nf, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            A.out[point] = traced ? make_float4(total[0] / nf, total[1] / nf, total[2] / nf, total[3] / nf) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

} // namespace rtk
