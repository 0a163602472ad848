// rt_vdenoise.hpp — the variance-guided A-trous filter (the spatial half of SVGF, Schied et al., HPG 2017, 4.2-4.4) over resultTexture
// or the temporal plane, guided by the feature planes of rt_render_aov (include/rt.h rt_denoise_variance).
//
// Definition (include/rt.h "variance-guided denoiser"; tests/vdenoise_oracle.c restates it in C): all float32, no FMA contraction, every
// quotient and sqrt correctly rounded, exp2_ = rtm::exp2_.  prep, kn, kz and zs are rt_denoise's (csrc/rt_denoise.hpp).
//   lum           l(e) = (0.2126 * e.x + 0.7152 * e.y) + 0.0722 * e.z
//   estimate      taps q = p + (dx, dy), dy = -3..3 outer, dx = -3..3 inner, a tap outside the image is skipped:
//                   g = exp2_(-(|G_p.xyz - G_q.xyz|^2 * kn + (G_p.w - G_q.w)^2 * zs))
//                 sg += g; m1 += g * l_q; m2 += g * (l_q * l_q) in tap order; mu = m1 / sg; v = m2 / sg - mu * mu; var_0 = v > 0 ? v : 0
//   pass i        s = 1 << i.  Prefilter: the 3 x 3 taps at spacing 1 that lie inside, dy outer, k3 = {1/4, 1/2, 1/4}:
//                   pn += (k3[dy + 1] * k3[dx + 1]) * var_i(q); pd += k3[dy + 1] * k3[dx + 1]; gv = pn / pd
//                 kl = 1 / (sigmaLuminance * sqrt(gv) + 1e-6).  Then rt_denoise's 25 taps at spacing s:
//                   x = (dn2 * kn + (dz * dz) * zs) + fabs(l(e_i(p)) - l(e_i(q))) * kl,  w = (h[dy + 2] * h[dx + 2]) * exp2_(-x)
//                 sw += w; s.ch += w * e_i(q).ch; sv += (w * w) * var_i(q); e_{i+1}(p).ch = s.ch / sw; var_{i+1}(p) = sv / (sw * sw)
//   output        out.ch = e_last.ch * d.ch, out.a = C.a
//
// k_denoise_prep (rt_denoise.hpp, unchanged) writes e0 and d.  k_variance_estimate reads e0 and writes (e0.rgb, var_0) into the other
// work plane and var_0 into the variance plane: variance rides in .w of the work planes, which k_atrous leaves unused, so a tap of a
// pass still costs two float4 loads (e_i(q) with its variance, G(q)).  The estimate writes a plane of its own and not e0.w in place: no
// lane then stores into a float4 another wave is loading.  k_var_atrous<LAST> is one launch per pass between the two work planes; the
// last pass multiplies by d and writes the denoised plane.  The 3 x 3 prefilter is nine .w loads inside the pass (rows y - 1 .. y + 1,
// which pass 0 loads anyway and which are the wave's own and its neighbours' cache lines in every pass): no plane and no launch of its
// own.  Workgroups, row and column handling are k_atrous's: 64 x 4 pixels, one image row per wave, a tap row outside the image is a
// wave-uniform branch, a column outside is a compare per lane, the skipped tap loads the centre column and its sums are kept by
// selects: no lane-divergent branch surrounds a load.  All taps are unrolled with compile-time weights (powers of two and 3/8: exact).
#pragma once
#include "rt_denoise.hpp"

namespace rtk {

struct VarEstimateArgs {
    const float4* e0;           // [H*W] e0.rgb (w unused)
    const float4* guide;        // [H*W] plane RT_AOV_NORMAL_DEPTH (n.xyz, z)
    float4* e_out;              // [H*W] (e0.rgb, var_0)
    float* var;                 // [H*W] var_0: the variance plane
    int W, H;
    float kn, kz;
};

struct VarAtrousArgs {
    const float4* e_in;         // [H*W] (e_i.rgb, var_i)
    const float4* guide;        // [H*W] plane RT_AOV_NORMAL_DEPTH (n.xyz, z)
    const float4* d;            // [H*W] (d.rgb, C.a): read by the last pass only
    float4* e_out;              // [H*W] (e_{i+1}.rgb, var_{i+1}), or the denoised plane in the last pass
    int W, H, step;
    float kn, kz, sl;           // sl = sigmaLuminance
};

__device__ __forceinline__ float vd_lum(const float4& e) { return (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z; }

__global__ __launch_bounds__(256) void k_variance_estimate(VarEstimateArgs a)
{
    const int x = blockIdx.x * kDenoiseTileW + (threadIdx.x & 63);
    const int y = blockIdx.y * kDenoiseTileH + (threadIdx.x >> 6);         // (one row per wave)
    if (y >= a.H || x >= a.W) return;
    const size_t W = (size_t)a.W;
    const size_t pi = (size_t)y * W + (size_t)x;
    const float4 ep = a.e0[pi], gp = a.guide[pi];
    const float zs = a.kz / (gp.w * gp.w + 1e-6f);
    const float kn = a.kn;
    float sg = 0.0f, m1 = 0.0f, m2 = 0.0f;
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.H) continue;                                  // (wave-uniform)
        const size_t row = (size_t)qy * W;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            const bool inside = qx >= 0 && qx < a.W;
            const size_t qi = row + (size_t)(inside ? qx : x);              // (a skipped tap loads the centre column: in bounds, unused)
            const float4 eq = a.e0[qi], gq = a.guide[qi];
            const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
            const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
            const float dz = gp.w - gq.w;
            const float g = rtm::exp2_(-(dn2 * kn + (dz * dz) * zs));
            const float lq = vd_lum(eq);
            sg = inside ? sg + g : sg;
            m1 = inside ? m1 + g * lq : m1;
            m2 = inside ? m2 + g * (lq * lq) : m2;
        }
    }
    const float mu = m1 / sg;
    const float v = m2 / sg - mu * mu;
    const float var0 = v > 0.0f ? v : 0.0f;
    a.e_out[pi] = make_float4(ep.x, ep.y, ep.z, var0);
    a.var[pi] = var0;
}

template <bool LAST>
__global__ __launch_bounds__(256) void k_var_atrous(VarAtrousArgs a)
{
    const int x = blockIdx.x * kDenoiseTileW + (threadIdx.x & 63);
    const int y = blockIdx.y * kDenoiseTileH + (threadIdx.x >> 6);         // (one row per wave)
    if (y >= a.H || x >= a.W) return;
    const size_t W = (size_t)a.W;
    const size_t pi = (size_t)y * W + (size_t)x;
    const float4 ep = a.e_in[pi], gp = a.guide[pi];
    const float zs = a.kz / (gp.w * gp.w + 1e-6f);
    const float kn = a.kn;
    const int s = a.step;
    // the 3 x 3 prefilter of the variance, spacing 1
    float pn = 0.0f, pd = 0.0f;
    constexpr float k3[3] = { 1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f };
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.H) continue;                                  // (wave-uniform)
        const size_t row = (size_t)qy * W;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            const bool inside = qx >= 0 && qx < a.W;
            const float vq = a.e_in[row + (size_t)(inside ? qx : x)].w;
            pn = inside ? pn + (k3[dy + 1] * k3[dx + 1]) * vq : pn;
            pd = inside ? pd + k3[dy + 1] * k3[dx + 1] : pd;
        }
    }
    const float gv = pn / pd;
    const float kl = 1.0f / (a.sl * __builtin_sqrtf(gv) + 1e-6f);
    const float lp = vd_lum(ep);
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
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
            const float xx = (dn2 * kn + (dz * dz) * zs) + __builtin_fabsf(lp - vd_lum(eq)) * kl;
            const float w = (h[dy + 2] * h[dx + 2]) * rtm::exp2_(-xx);
            sw = inside ? sw + w : sw;
            sx = inside ? sx + w * eq.x : sx; sy = inside ? sy + w * eq.y : sy; sz = inside ? sz + w * eq.z : sz;
            sv = inside ? sv + (w * w) * eq.w : sv;
        }
    }
    float4 o = make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
    if (LAST) {
        const float4 dv = a.d[pi];
        o.x = o.x * dv.x; o.y = o.y * dv.y; o.z = o.z * dv.z; o.w = dv.w;
    }
    a.e_out[pi] = o;
}

} // namespace rtk
