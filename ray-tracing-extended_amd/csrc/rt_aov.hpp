// rt_aov.hpp — first-hit feature buffers (include/rt.h rt_render_aov): per pixel the albedo, shading normal, depth and coverage of the
// first visible surface, averaged over the frame's NumRaysPerPixel camera rays and accumulated over feature frames — what a denoiser
// or an edge-aware filter takes beside the noisy image.
//
// Definition (include/rt.h "feature buffers"; tests/aov_oracle.c restates it in C):
//   camera rays   sample s of pixel (x, y) of frame f draws its ray as frag :377-382 does, from the Philox stream key (pixelIndex, f),
//                 counter (block 0, sample s) whatever rngMode is — in Philox mode the very rays the frame traces
//   surface       the hit at which Trace (:300-352) first scatters: the first hit, except that an InvisibleLight (flag 2) is passed
//                 through once as Trace does at bounce 0 (origin = hitPoint + dir * 0.001, one more cast, only if MaxBounceCount >= 1)
//   sum           the estimator's tree of the Philox mode, each of the eight channels on its own; root / NumRaysPerPixel
//   accumulate    acc * (1 - w) + cur * w, w = 1 / (k + 1), k = feature frames so far; no saturate (normals are signed)
//
// One launch per frame, no persistent loop.  A pixel's S = 16 / 4 / 1 sub-streams sit on S ADJACENT lanes of a wave (lane = pixel * S +
// sub-stream; a wave is 2x2 / 4x4 / 8x8 pixels), lane k walks samples k, k + S, ...: one camera ray, one closest_hit (two on a
// pass-through) and eight adds each.  The tree is then four xor-exchanges per channel at lane distances 1, 2, 4, 8 — inside a row of 16
// lanes, so each is a DPP move or a swizzle, no LDS traffic — and the sub-stream-0 lane reads the pixel's two accumulators, blends and
// stores them.  The traversal stack is k_ray_query's: tile_stack_cap entries per lane in LDS, the rest in the global overflow area.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

struct AovArgs {
    rt_params p;
    int frame;
    int accumulated;            // feature frames in the planes before this one (the blend weight is 1 / (accumulated + 1))
    int row0, nrows, row_stride;    // as FrameArgs: local row ly -> global row row0 + (ly / 8) * row_stride + ly % 8
    int tiles_x, ntiles;        // a wave's tile is 2^t x 2^t pixels, t = (6 - sample_lanes_log2) / 2
    int sample_lanes_log2;      // log2 S
    int stack_cap, full_sort, fixed_origin;     // as FrameArgs
    uint32_t* gstack; unsigned int gstack_stride;
    float4* albedo;             // [nrows*W] (albedo.rgb, coverage)
    float4* normal_depth;       // [nrows*W] (normal.xyz, depth)
};

template <bool H>
__global__ __launch_bounds__(kBlock) void k_aov(DeviceScene S, AovArgs A)
{
    extern __shared__ uint32_t lds_stack[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int tile = blockIdx.x * kWavesPerBlock + wave;
    if (tile >= (unsigned)A.ntiles) return;                             // (wave-uniform)
    const TravStack stk = lane_stack(lds_stack, A.stack_cap, A.gstack, A.gstack_stride);

    const rt_params& p = A.p;
    const int sl = A.sample_lanes_log2, tl = (6 - sl) >> 1;
    const int nsub = 1 << sl;
    const unsigned int pix = (unsigned)lane >> sl;
    const int sub = lane & (nsub - 1);
    const int tx = (int)(tile % (unsigned)A.tiles_x), ty = (int)(tile / (unsigned)A.tiles_x);
    const int x = (tx << tl) + (int)(pix & ((1u << tl) - 1u)), ly = (ty << tl) + (int)(pix >> tl);
    const bool present = x < p.width && ly < A.nrows;
    const int y = A.row0 + (ly >> 3) * A.row_stride + (ly & 7);
    const uint32_t W = (uint32_t)p.width;
    const uint32_t pixelIndex = (uint32_t)y * W + (uint32_t)x;

    Camera cam;
    cam.W = (float)W;
    {
        const float* M = p.camLocalToWorld;
        const float uvx = ((float)x + 0.5f) / cam.W, uvy = ((float)y + 0.5f) / (float)(uint32_t)p.height;
        const float lx = (uvx - 0.5f) * p.viewParams[0], lyv = (uvy - 0.5f) * p.viewParams[1], lz = 1.0f * p.viewParams[2];
        cam.focusPoint = rtm::mk(((M[0] * lx + M[1] * lyv) + M[2]  * lz) + M[3]  * 1.0f,
                                 ((M[4] * lx + M[5] * lyv) + M[6]  * lz) + M[7]  * 1.0f,
                                 ((M[8] * lx + M[9] * lyv) + M[10] * lz) + M[11] * 1.0f);
        cam.right = rtm::mk(M[0], M[4], M[8]);
        cam.up    = rtm::mk(M[1], M[5], M[9]);
        cam.pos   = ld3(p.worldSpaceCameraPos);
    }

    // this lane's sub-stream: samples sub, sub + S, ... in increasing order, starting from 0.  A flat loop, one closest_hit per trip
    // (render_pixel's shape): a pass-through repeats the trip with the moved origin.  Hit or miss is h.id, a value, never a carried bool.
    v3 alb = rtm::mk(0.f, 0.f, 0.f), nrm = rtm::mk(0.f, 0.f, 0.f);
    float cov = 0.f, dep = 0.f;
    Counters cnt = {};
    const bool full_sort = A.full_sort != 0, fixed_origin = A.fixed_origin != 0;
    int sample = sub, cast = 0;
    bool alive = present && sample < p.numRaysPerPixel && p.maxBounceCount >= 0;    // (Trace casts MaxBounceCount + 1 rays at most: none, no surface)
    v3 o, d, origin;
    if (alive) {
        rtm::PhiloxScope R;
        R.begin(pixelIndex, (uint32_t)A.frame, (uint32_t)sample, 0u);
        camera_ray(p, cam, R, o, d, fixed_origin);
        origin = o;
    }
    while (alive) {
        const Hit h = closest_hit<false, H>(S, p.intersectMode, full_sort, o, d, stk, cnt);
        bool sample_done = true;
        if (h.id != kNone) {
            const v3 hitPoint = o + d * h.t;
            v3 normal; const float4* mat;
            surface_of(S, h, hitPoint, normal, mat);
            const float4 mcol = mat[0], mprm = mat[3];
            const int flag = (int)__float_as_uint(mprm.w);
            if (flag == 2 && cast == 0) {                                   // InvisibleLightSource :318-322
                // with no bounce left Trace ends behind the light without scattering: the sample has no surface
                if (p.maxBounceCount >= 1) { o = hitPoint + d * 0.001f; cast = 1; sample_done = false; }
            } else {
                v3 colour = rtm::mk(mcol.x, mcol.y, mcol.z);
                if (flag == 1) {                                            // CheckerPattern :313-317
                    const float cx = mod2(__builtin_floorf(hitPoint.x)), cz = mod2(__builtin_floorf(hitPoint.z));
                    if (!(cx == cz)) { const float4 memi = mat[1]; colour = rtm::mk(memi.x, memi.y, memi.z); }
                }
                const v3 q = hitPoint - origin;
                alb = alb + colour; cov = cov + 1.0f;
                nrm = nrm + normal; dep = dep + rtm::sqrt_(rtm::dot(q, q));
            }
        }
        if (sample_done) {
            sample += nsub; cast = 0;
            if (sample >= p.numRaysPerPixel) alive = false;
            else {
                rtm::PhiloxScope R;
                R.begin(pixelIndex, (uint32_t)A.frame, (uint32_t)sample, 0u);
                camera_ray(p, cam, R, o, d, fixed_origin);
                origin = o;
            }
        }
    }

    // the estimator's tree: (k, k + 1) for even k, then (k, k + 2) for k = 0 mod 4, ...; lanes without a pixel carry zeros and every lane
    // of the wave takes part in the exchanges
    for (int off = 1; off < nsub; off <<= 1) {
        alb.x = alb.x + __shfl_xor(alb.x, off, 64); alb.y = alb.y + __shfl_xor(alb.y, off, 64); alb.z = alb.z + __shfl_xor(alb.z, off, 64);
        cov = cov + __shfl_xor(cov, off, 64);
        nrm.x = nrm.x + __shfl_xor(nrm.x, off, 64); nrm.y = nrm.y + __shfl_xor(nrm.y, off, 64); nrm.z = nrm.z + __shfl_xor(nrm.z, off, 64);
        dep = dep + __shfl_xor(dep, off, 64);
    }
    if (present && sub == 0) {
        const float nf = (float)p.numRaysPerPixel;
        const float weight = 1.0f / (float)(A.accumulated + 1), omw = 1.0f - weight;
        const size_t pi = (size_t)ly * W + (uint32_t)x;
        const float4 pa = A.albedo[pi], pn = A.normal_depth[pi];
        float4 a, n;
        a.x = pa.x * omw + (alb.x / nf) * weight; a.y = pa.y * omw + (alb.y / nf) * weight;
        a.z = pa.z * omw + (alb.z / nf) * weight; a.w = pa.w * omw + (cov / nf) * weight;
        n.x = pn.x * omw + (nrm.x / nf) * weight; n.y = pn.y * omw + (nrm.y / nf) * weight;
        n.z = pn.z * omw + (nrm.z / nf) * weight; n.w = pn.w * omw + (dep / nf) * weight;
        A.albedo[pi] = a; A.normal_depth[pi] = n;
    }
}

} // namespace rtk
