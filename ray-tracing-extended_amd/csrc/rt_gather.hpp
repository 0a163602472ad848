// rt_gather.hpp — gather queries: the light that arrives at a POINT, over the cosine lobe about its normal or over the sphere as nine SH
// coefficients (include/rt.h rt_gather).  What a lightmap texel or a light probe asks; the directions are drawn on the device.
//
// Definition (include/rt.h "gather queries"; tests/query_oracle.c runs the oracle's own random_direction() and trace() for it):
//   stream        point i of a call has the Philox key (firstIndex + i, seed); sample s draws its direction from counter (block, s) with
//                 blocks 0xFFFFFFFE (words 0..3) and 0xFFFFFFFF (words 0, 1): R = RandomDirection (RayTracing.shader:216-223).  Trace's
//                 hits use blocks 1 + 2b, 2 + 2b as in a radiance query, so the two never meet
//   direction     RT_GATHER_COSINE: d = normalize(n + R) (:328's expression, n as given); RT_GATHER_SH9: d = R
//   sample        L_s = Trace(origin, d) as a radiance query runs it: the cast at loop index 0 bounded by tMax, every later one unbounded
//   sum           the Philox mode's tree over the N samples; COSINE: one float4 (root.rgb / N, 1); SH9: nine float4, the tree over
//                 L_s.c * Y_k(d), (root / N) * 4 pi, w = 1 for k = 0 and 0 otherwise.  tMax <= 0 or NaN: zeros, no draw, no cast
//
// The launch, the lane layout (an item is a point) and the estimator's tree are the sample-lane frame's (rt_sampled.hpp).  The loop is
// k_aov's: flat, ONE closest_hit site per trip, then the shading of that hit.  Every sample has its own first cast (there is nothing
// for k_radiance's first-cast reuse to keep): the direction of a lane's next sample is drawn in the step that ends its path, and once
// before the loop.  The point is read again from memory there instead of living in seven registers across the loop.
//
// The shading step is k_radiance's, expression for expression, COPIED.  Sharing it was tried: one __forceinline__ function for the hit
// (:309-343) that both kernels call, k_radiance handing its entry bookkeeping (e_h / e_o / e_bounce) in as a callback that runs once the
// material's flag is read.  k_radiance's code object changed with it: 3049 -> 3061 and 3055 -> 3067 instructions, and the f32-node
// instantiation went from 109 to 111 VGPRs (tools/kernel_resources.py), so the kernels keep a copy each.  A second form, the step
// as two functions with k_radiance's bookkeeping between them in its own body, cost no instruction and no register in any instantiation
// but reordered 109 / 79 positions of k_radiance and 9 / 17 of k_gather, untimed: not kept (profiles/sampled_frame_notes.txt).
// A change to one is a change to both; tests/test_gpu_gather.py holds N = 1 of this kernel bitwise to k_radiance.
#pragma once
#include "rt_sampled.hpp"

namespace rtk {

struct GatherArgs : ShadingHead, SampledHead {      // in: the points, (normal, -) second; out: [n] (COSINE) or [n*9] (SH9)
    int sample_lanes_log2;      // log2 S
    int stack_cap, full_sort;   // as QueryArgs
    uint32_t* gstack; unsigned int gstack_stride;
};
static_assert(sizeof(SampledHead) == 32 && sizeof(GatherArgs) == sizeof(rt_params) + 64, "a kernel argument moved");

constexpr uint32_t kGatherBlock = 0xFFFFFFFEu;     // first Philox block of a sample's direction draw

// the direction of sample `sample` of the point with key `key` and normal n
template <int MODE>
__device__ __forceinline__ v3 gather_direction(uint32_t key, uint32_t seed, uint32_t sample, const v3& n)
{
    rtm::PhiloxScope R;
    R.begin(key, seed, sample, kGatherBlock);
    const v3 r = rtm::random_direction(R);
    if (MODE == RT_GATHER_SH9) return r;
    return rtm::normalize(n + r);                                       // :328's diffuse lobe
}

template <int MODE, bool H>
__global__ __launch_bounds__(kBlock) void k_gather(DeviceScene S, GatherArgs A)
{
    extern __shared__ uint32_t lds_stack[];
    constexpr int NC = MODE == RT_GATHER_SH9 ? 9 : 1;                   // float4 per point
    const SampleLane L = sample_lane(A);
    if (L.idle_wave) return;
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);
    const rt_params& p = A.p;

    v3 o = rtm::mk(0.f, 0.f, 0.f), d = o;
    float t_bound = 0.0f;
    if (L.present) {
        const float4 r0 = A.in[2 * (size_t)L.item];
        o = rtm::mk(r0.x, r0.y, r0.z);
        t_bound = r0.w;
    }
    const bool traced = t_bound > 0.0f;                                 // tMax <= 0 or NaN: zeros, nothing drawn or traced
    const uint32_t key = A.first_index + L.item;                        // first Philox key word: the item's index in the call's stream

    v3 total[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) total[k] = rtm::mk(0.f, 0.f, 0.f);
    v3 rayColour = rtm::mk(1.f, 1.f, 1.f), light = rtm::mk(0.f, 0.f, 0.f);
    v3 d_first = d;                                                     // the sample's drawn direction (SH9: the basis is evaluated on it)
    int sample = L.sub, bounce = 0;
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0;
    bool alive = L.present && traced && sample < A.samples && p.maxBounceCount >= 0;   // (Trace casts MaxBounceCount + 1 rays at most)
    if (alive) {
        const float4 r1 = A.in[2 * (size_t)L.item + 1];
        d = gather_direction<MODE>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
        if (MODE == RT_GATHER_SH9) d_first = d;
    }

    while (alive) {
        const Hit h = closest_hit<false, H>(S, p.intersectMode, full_sort, o, d, stk, cnt, t_bound);
        t_bound = __builtin_inff();                                     // only the cast at loop index 0 is bounded
        bool path_done;
        if (h.id != kNone) {
            // ---- hit: Trace :309-343 (k_radiance's expressions)
            const v3 hitPoint = o + d * h.t;
            v3 normal; const float4* mat;
            surface_of(S, h, hitPoint, normal, mat);
            const float4 mcol = mat[0], memi = mat[1], mprm = mat[3];
            const int flag = (int)__float_as_uint(mprm.w);
            v3 colour = rtm::mk(mcol.x, mcol.y, mcol.z);
            bool skip = false;
            if (flag == 1) {                                                           // CheckerPattern :313-317
                const float cx = mod2(__builtin_floorf(hitPoint.x)), cz = mod2(__builtin_floorf(hitPoint.z));
                if (!(cx == cz)) colour = rtm::mk(memi.x, memi.y, memi.z);
            } else if (flag == 2 && bounce == 0) skip = true;                          // InvisibleLightSource :318-322
            path_done = false;
            if (skip) o = hitPoint + d * 0.001f;
            else {
                rtm::PhiloxScope R;                                                    // the eight draws of this hit: blocks 1 + 2b, 2 + 2b
                R.begin(key, A.seed, (uint32_t)sample, 1u + 2u * (uint32_t)bounce);
                const bool isSpecular = mprm.z >= rtm::random_value(R);                // :325
                const float specF = isSpecular ? 1.0f : 0.0f;
                o = hitPoint;                                                          // :327
                const v3 diffuseDir = rtm::normalize(normal + rtm::random_direction(R));
                const float4 mspec = mat[2];
                const v3 specularDir = rtm::reflect(d, normal);
                d = rtm::normalize(rtm::lerp(diffuseDir, specularDir, mprm.y * specF));
                const v3 emitted = rtm::mk(memi.x, memi.y, memi.z) * mprm.x;           // :333-335
                light = light + emitted * rayColour;
                rayColour = rayColour * rtm::lerp(colour, rtm::mk(mspec.x, mspec.y, mspec.z), specF);
                const float pr = rtm::fmax_(rayColour.x, rtm::fmax_(rayColour.y, rayColour.z));   // :338-342
                if (rtm::random_value(R) >= pr) path_done = true;
                else { const float ip = rtm::rcp_(pr); rayColour = rayColour * ip; }
            }
            ++bounce;
            if (bounce > p.maxBounceCount) path_done = true;                           // loop bound :305
        } else {
            light = light + environment_light(p, d) * rayColour;                       // :346-347
            path_done = true;
        }
        if (path_done) {
            if (MODE == RT_GATHER_SH9) {
                float Y[9];
                sh9_basis(d_first, Y);
#pragma unroll
                for (int k = 0; k < NC; ++k) total[k] = total[k] + light * Y[k];
            } else total[0] = total[0] + light;
            sample += L.nsub;
            if (sample >= A.samples) alive = false;
            else {
                // the next sample starts at the point again, along a direction of its own, its first cast bounded
                const float4 r0 = A.in[2 * (size_t)L.item], r1 = A.in[2 * (size_t)L.item + 1];
                o = rtm::mk(r0.x, r0.y, r0.z);
                t_bound = r0.w;
                d = gather_direction<MODE>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
                if (MODE == RT_GATHER_SH9) d_first = d;
                bounce = 0;
                rayColour = rtm::mk(1.f, 1.f, 1.f); light = rtm::mk(0.f, 0.f, 0.f);
            }
        }
    }

    tree_sum<3 * NC>(&total[0].x, L.nsub);                              // (a v3 is its three floats)
    if (L.stores()) {
        const float nf = (float)A.samples;
        float4* out = A.out + (size_t)NC * L.item;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (!traced) { out[k] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
            const v3 m = rtm::mk(total[k].x / nf, total[k].y / nf, total[k].z / nf);
            out[k] = MODE == RT_GATHER_SH9 ? make_float4(m.x * 12.566371f, m.y * 12.566371f, m.z * 12.566371f, k == 0 ? 1.0f : 0.0f)
                                           : make_float4(m.x, m.y, m.z, 1.0f);
        }
    }
}

} // namespace rtk
