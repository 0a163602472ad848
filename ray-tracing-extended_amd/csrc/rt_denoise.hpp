// rt_denoise.hpp — edge-avoiding A-trous wavelet filter (Dammertz et al., HPG 2010) over resultTexture, guided by the feature planes
// of rt_render_aov, with albedo demodulation (include/rt.h rt_denoise).
//
// Definition (include/rt.h "denoiser"; tests/denoise_oracle.c restates it in C): all float32, no FMA contraction, every quotient
// correctly rounded, exp2_ = rtm::exp2_.
//   prep          cov1 = 1 - A.w; d.ch = max(A.ch + cov1, 0.01) (demodulate == 0: d = 1); e0.ch = C.ch / d.ch
//   pass i        s = 1 << i; taps q = p + (dx * s, dy * s), dy = -2..2 outer, dx = -2..2 inner, a tap outside the image is skipped:
//                   x = (|G_p.xyz - G_q.xyz|^2 * kn + (G_p.w - G_q.w)^2 * zs) + |e_i(p) - e_i(q)|^2 * kc_i,  zs = kz / (G_p.w^2 + 1e-6)
//                   w = (h[dy + 2] * h[dx + 2]) * exp2_(-x),  h = {1/16, 1/4, 3/8, 1/4, 1/16}
//                 sw += w; s.ch += w * e_i(q).ch in tap order; e_{i+1}(p).ch = s.ch / sw
//   output        out.ch = e_last.ch * d.ch, out.a = C.a
//
// k_denoise_prep writes e0 and d once (C.a rides in d.w), so a tap costs two float4 loads: e_i(q) and G(q).  k_atrous<LAST> is one
// launch per pass, ping-ponging between two work planes; the last pass multiplies by d and writes the denoised plane.  A workgroup is
// 64 x 4 pixels, one image row per wave: a tap row is 1 KiB contiguous per wave, "is this tap's row inside" is wave-uniform (a scalar
// branch around five taps) and "is its column inside" one compare per lane: a skipped tap loads the centre column instead and its sums
// are kept by selects, so the ten loads of a tap row are issued together, with no lane-divergent branch.  The 25 taps are unrolled; the
// weights h[dy] * h[dx] are compile-time constants (products of powers of two and 3/8: exact).
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

constexpr int kDenoiseTileW = 64, kDenoiseTileH = 4;

struct AtrousArgs {
    const float4* e_in;         // [H*W] e_i.rgb (w unused)
    const float4* guide;        // [H*W] plane RT_AOV_NORMAL_DEPTH (n.xyz, z)
    const float4* d;            // [H*W] (d.rgb, C.a): read by the last pass only
    float4* e_out;              // [H*W] e_{i+1}, or the denoised plane in the last pass
    int W, H, step;
    float kn, kz, kc;
};

__global__ __launch_bounds__(256) void k_denoise_prep(const float4* __restrict__ C, const float4* __restrict__ A, float4* __restrict__ e0,
                                                      float4* __restrict__ d, size_t n, int demodulate)
{
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = C[i];
    float4 dv = make_float4(1.0f, 1.0f, 1.0f, c.w), e = c;
    if (demodulate) {
        const float4 a = A[i];
        const float cov1 = 1.0f - a.w;
        const float tx = a.x + cov1, ty = a.y + cov1, tz = a.z + cov1;
        dv.x = tx > 0.01f ? tx : 0.01f; dv.y = ty > 0.01f ? ty : 0.01f; dv.z = tz > 0.01f ? tz : 0.01f;
        e.x = c.x / dv.x; e.y = c.y / dv.y; e.z = c.z / dv.z;
    }
    e0[i] = e; d[i] = dv;
}

template <bool LAST>
__global__ __launch_bounds__(256) void k_atrous(AtrousArgs a)
{
    const int x = blockIdx.x * kDenoiseTileW + (threadIdx.x & 63);
    const int y = blockIdx.y * kDenoiseTileH + (threadIdx.x >> 6);         // (one row per wave)
    if (y >= a.H || x >= a.W) return;
    const size_t W = (size_t)a.W;
    const size_t pi = (size_t)y * W + (size_t)x;
    const float4 ep = a.e_in[pi], gp = a.guide[pi];
    const float zs = a.kz / (gp.w * gp.w + 1e-6f);
    const float kn = a.kn, kc = a.kc;
    const int s = a.step;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    constexpr float h[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= a.H) continue;                                  // (wave-uniform)
        const size_t row = (size_t)qy * W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const bool inside = qx >= 0 && qx < a.W;
            const size_t qi = row + (size_t)(inside ? qx : x);              // (a skipped tap loads the centre column: in bounds, unused)
            const float4 eq = a.e_in[qi], gq = a.guide[qi];
            const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
            const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
            const float dz = gp.w - gq.w;
            const float dcx = ep.x - eq.x, dcy = ep.y - eq.y, dcz = ep.z - eq.z;
            const float dc2 = (dcx * dcx + dcy * dcy) + dcz * dcz;
            const float xx = (dn2 * kn + (dz * dz) * zs) + dc2 * kc;
            const float w = (h[dy + 2] * h[dx + 2]) * rtm::exp2_(-xx);
            sw = inside ? sw + w : sw;
            sx = inside ? sx + w * eq.x : sx; sy = inside ? sy + w * eq.y : sy; sz = inside ? sz + w * eq.z : sz;
        }
    }
    float4 o = make_float4(sx / sw, sy / sw, sz / sw, 0.0f);
    if (LAST) {
        const float4 dv = a.d[pi];
        o.x = o.x * dv.x; o.y = o.y * dv.y; o.z = o.z * dv.z; o.w = dv.w;
    }
    a.e_out[pi] = o;
}

} // namespace rtk
