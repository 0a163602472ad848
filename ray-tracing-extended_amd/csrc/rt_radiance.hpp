// rt_radiance.hpp — radiance queries: Trace (RayTracing.shader:300-352) for rays the caller supplies (include/rt.h rt_trace_radiance):
// how much light arrives along each ray, averaged over N independent runs of Trace.
//
// Definition (include/rt.h "radiance queries"; tests/query_oracle.c runs the oracle's own trace() for it):
//   stream        ray i of a call has the Philox key (firstIndex + i, seed); sample s draws from counter (block, s): the hit at loop index
//                 b takes blocks 1 + 2b and 2 + 2b, block 0 (a frame's camera ray) is unused — the caller made the ray
//   first cast    counts only hits with dst < tMax (rt_trace_rays' rule); every later cast is unbounded
//   sum           the estimator's tree of the Philox mode over the N samples, root / N; alpha 1.  tMax <= 0 or NaN: four zeros, no cast
//
// The launch, the lane layout (an item is a ray) and the estimator's tree are the sample-lane frame's (rt_sampled.hpp).  A flat state
// machine shaped like render_pixel / k_aov: one closest_hit per trip, then the shading of that hit; sample and bounce advance in the
// same loop.
//
// First-cast reuse.  What Trace does before its first draw depends on the ray alone: the bounded cast at loop index 0 and, when that
// hits an InvisibleLight (flag 2) with a bounce left, the pass-through cast from hitPoint + dir * 0.001.  A lane makes these casts once,
// keeps the answer — the "entry": origin, loop index and Hit of the last ray-only cast — and every further sample of the lane re-enters
// the shading step from it without a traversal (closest_hit is a function of its arguments, so the repeated cast would return these
// bits).  At N = 64, S = 16 that removes three of each lane's four first casts.
#pragma once
#include "rt_sampled.hpp"

namespace rtk {

struct RadianceArgs : ShadingHead, SampledHead {    // in: the rays; out: [n] rgba
    int sample_lanes_log2;      // log2 S
    int stack_cap, full_sort;   // as QueryArgs
    uint32_t* gstack; unsigned int gstack_stride;
};
static_assert(sizeof(SampledHead) == 32 && sizeof(RadianceArgs) == sizeof(rt_params) + 64, "a kernel argument moved");

template <bool H>
__global__ __launch_bounds__(kBlock) void k_radiance(DeviceScene S, RadianceArgs A)
{
    extern __shared__ uint32_t lds_stack[];
    const SampleLane L = sample_lane(A);
    if (L.idle_wave) return;
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);
    const rt_params& p = A.p;

    v3 o = rtm::mk(0.f, 0.f, 0.f), d0 = o;
    float t_bound = 0.0f;
    if (L.present) {
        const float4 r0 = A.in[2 * (size_t)L.item], r1 = A.in[2 * (size_t)L.item + 1];
        o = rtm::mk(r0.x, r0.y, r0.z); d0 = rtm::mk(r1.x, r1.y, r1.z);
        t_bound = r0.w;
    }
    const bool traced = t_bound > 0.0f;                                 // tMax <= 0 or NaN: four zeros, nothing traced
    const uint32_t key = A.first_index + L.item;                        // first Philox key word: the item's index in the call's stream

    v3 total = rtm::mk(0.f, 0.f, 0.f);
    v3 d = d0, rayColour = rtm::mk(1.f, 1.f, 1.f), light = rtm::mk(0.f, 0.f, 0.f);
    int sample = L.sub, bounce = 0;
    // the entry (file header): set at the first shading step that is not a pass-through with a cast to follow
    Hit e_h; e_h.t = 0.f; e_h.id = kNone; e_h.u = 0.f; e_h.v = 0.f;
    v3 e_o = o;
    int e_bounce = -1;                                                  // -1: not set yet
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0;
    bool alive = L.present && traced && sample < A.samples && p.maxBounceCount >= 0;   // (Trace casts MaxBounceCount + 1 rays at most)

    while (alive) {
        Hit h = closest_hit<false, H>(S, p.intersectMode, full_sort, o, d, stk, cnt, t_bound);
        t_bound = __builtin_inff();                                     // only the cast at loop index 0 is bounded
        bool again;
        do {
            again = false;
            bool path_done;
            if (h.id != kNone) {
                // ---- hit: Trace :309-343 (render_pixel's expressions)
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
                // with no bounce left the pass-through ends the path without a cast: this step is the entry after all
                if (e_bounce < 0 && !(skip && p.maxBounceCount >= 1)) { e_h = h; e_o = o; e_bounce = bounce; }
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
                if (e_bounce < 0) { e_h = h; e_o = o; e_bounce = bounce; }
                light = light + environment_light(p, d, true) * rayColour;                 // :346-347 (d may be the caller's: any length)
                path_done = true;
            }
            if (path_done) {
                total = total + light;
                sample += L.nsub;
                if (sample >= A.samples) alive = false;
                else {
                    // the next sample re-enters at the entry: no cast
                    h = e_h; o = e_o; d = d0; bounce = e_bounce;
                    rayColour = rtm::mk(1.f, 1.f, 1.f); light = rtm::mk(0.f, 0.f, 0.f);
                    again = true;
                }
            }
        } while (again);
    }

    float sum[3] = { total.x, total.y, total.z };
    tree_sum<3>(sum, L.nsub);
    if (L.stores()) {
        const float nf = (float)A.samples;
        A.out[L.item] = traced ? make_float4(sum[0] / nf, sum[1] / nf, sum[2] / nf, 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

} // namespace rtk
