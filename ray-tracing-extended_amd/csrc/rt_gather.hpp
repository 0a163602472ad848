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
// One launch per slice of points, no persistent loop.  A point's S = 16 / 4 / 1 sub-streams sit on S ADJACENT lanes (lane = point * S +
// sub-stream), lane k walks samples k, k + S, ...  The loop is k_aov's: flat, ONE closest_hit site per trip, then the shading of that
// hit.  Every sample has its own first cast (there is nothing for k_radiance's first-cast reuse to keep): the direction of a lane's next
// sample is drawn in the step that ends its path, and once before the loop, so lanes meet again at the traversal whatever their path
// lengths.  The point is read again from memory there instead of living in seven registers across the loop.
//
// The shading step is k_radiance's, expression for expression, COPIED.  Sharing it was tried: one __forceinline__ function for the hit
// (:309-343) that both kernels call, k_radiance handing its entry bookkeeping (e_h / e_o / e_bounce) in as a callback that runs once the
// material's flag is read.  k_radiance's code object changed with it: 3049 -> 3061 and 3055 -> 3067 instructions, and the f32-node
// instantiation went from 109 to 111 VGPRs (tools/kernel_resources.py), so the kernels keep a copy each.  A change to one is a change
// to both; tests/test_gpu_gather.py holds N = 1 of this kernel bitwise to k_radiance.
//
// The tree is four xor-exchanges per channel at lane distances 1, 2, 4, 8; every lane of the wave takes part, lanes without a point
// carry zeros, and the sub-stream-0 lane stores one or nine float4.  Hit or miss is carried as h.id, a value, never as a bool across
// the traversal (rt_kernels.hpp, the per-lane walk, records why).
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

struct GatherArgs {
    rt_params p;                // the settings that apply: maxBounceCount, intersectMode, the environment
    const float4* points;       // [n*2]  rt_ray: (origin, tMax) (normal, -)
    float4* out;                // [n] (COSINE) or [n*9] (SH9)
    int n;
    int samples;                // N
    uint32_t seed;              // second key word
    uint32_t first_index;       // first key word of point 0 of this launch
    int sample_lanes_log2;      // log2 S
    int stack_cap, full_sort;   // as QueryArgs
    uint32_t* gstack; unsigned int gstack_stride;
};

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
    const int sl = A.sample_lanes_log2, nsub = 1 << sl;
    const unsigned int g = blockIdx.x * kBlock + threadIdx.x;          // (the host keeps points-per-launch * S below 2^31)
    if ((g & ~63u) >> sl >= (unsigned)A.n) return;                      // (wave-uniform: no lane of this wave has a point)
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);
    const rt_params& p = A.p;
    const unsigned int point = g >> sl;
    const int sub = (int)(g & (unsigned)(nsub - 1));
    const bool present = point < (unsigned)A.n;

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
    v3 total[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) total[k] = rtm::mk(0.f, 0.f, 0.f);
    v3 rayColour = rtm::mk(1.f, 1.f, 1.f), light = rtm::mk(0.f, 0.f, 0.f);
    v3 d_first = d;                                                     // the sample's drawn direction (SH9: the basis is evaluated on it)
    int sample = sub, bounce = 0;
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0;
    bool alive = present && traced && sample < A.samples && p.maxBounceCount >= 0;     // (Trace casts MaxBounceCount + 1 rays at most)
    if (alive) {
        const float4 r1 = A.points[2 * (size_t)point + 1];
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
                // the real SH basis of bands 0..2 on the drawn direction, every product its own rounding (include/rt.h)
                const float x = d_first.x, y = d_first.y, z = d_first.z;
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
                for (int k = 0; k < NC; ++k) total[k] = total[k] + light * Y[k];
            } else total[0] = total[0] + light;
            sample += nsub;
            if (sample >= A.samples) alive = false;
            else {
                // the next sample starts at the point again, along a direction of its own, its first cast bounded
                const float4 r0 = A.points[2 * (size_t)point], r1 = A.points[2 * (size_t)point + 1];
                o = rtm::mk(r0.x, r0.y, r0.z);
                t_bound = r0.w;
                d = gather_direction<MODE>(key, A.seed, (uint32_t)sample, rtm::mk(r1.x, r1.y, r1.z));
                if (MODE == RT_GATHER_SH9) d_first = d;
                bounce = 0;
                rayColour = rtm::mk(1.f, 1.f, 1.f); light = rtm::mk(0.f, 0.f, 0.f);
            }
        }
    }

    // the estimator's tree: (k, k + 1) for even k, then (k, k + 2) for k = 0 mod 4, ...
    for (int off = 1; off < nsub; off <<= 1) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            total[k].x = total[k].x + __shfl_xor(total[k].x, off, 64);
            total[k].y = total[k].y + __shfl_xor(total[k].y, off, 64);
            total[k].z = total[k].z + __shfl_xor(total[k].z, off, 64);
        }
    }
    if (present && sub == 0) {
        const float nf = (float)A.samples;
        float4* out = A.out + (size_t)NC * point;
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
