// rt_temporal.hpp — temporal reprojection of the image of a moving camera (include/rt.h rt_temporal): the step between resultTexture
// and rt_denoise, the temporal stage of SVGF (Schied et al., HPG 2017) without its variance estimate.
//
// Definition (include/rt.h "temporal reprojection"; tests/temporal_oracle.c restates it in C): all float32, no FMA contraction, every
// quotient and sqrt correctly rounded, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, normalize = rtm::normalize.
//   surface       cov = A.w; surf = cov > 0; nc = G.xyz / cov, zc = G.w / cov (0 without a surface)
//   centre ray    frag's ray without jitter: dir = normalize(M * (l, 1) - O), l = ((uv.x - .5) * V.x, (uv.y - .5) * V.y, V.z)
//   point         surface: X = O + dir * zc, q = X - t', ze = sqrt(dot(X - O', X - O')); sky: q = dir
//   previous view l'_i = dot(c_i, q) / dot(c_i, c_i); l'_z > 0; px = ((l'_x * (V'.z / l'_z)) / V'.x + .5) * W - .5, -1 < px < W (py alike)
//   taps          (floor(px) + i, floor(py) + j), j outer, bilinear weight b; a tap counts inside the image, with N' > 0 and a guide
//                 that agrees (surface: G'.w > 0, |G'.w - ze| <= depthTolerance * ze, |nc - G'.xyz|^2 <= normalTolerance^2; sky: G'.w == 0)
//   blend         sw >= 0.01: n = min(hn / sw + 1, maxHistory), T = (h / sw) * (1 - 1/n) + C * (1/n); else n = 1, T = C
//
// One launch per call.  A workgroup is 64 x 4 pixels, one image row per wave (the denoiser's layout): the centre reads of C, A and G
// are 1 KiB contiguous per wave.  The four taps are a gather: for a small camera motion the lanes of a wave land in one or two rows of
// T', N' and G'.  A tap outside the image, and every tap of a pixel whose reprojection failed, loads the pixel's own address instead
// (in bounds, unused); whether a tap counts is decided from what was loaded, by selects, so the twelve tap loads are issued together
// behind one wait and no lane-divergent branch surrounds a load.  The previous camera and every constant are kernel arguments,
// computed by the host in float32 as the header says.  T, N and G' are ping-pong pairs: the step never reads a plane it writes.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

constexpr int kTemporalTileW = 64, kTemporalTileH = 4;

struct TemporalArgs {
    const float4* C;            // [H*W] resultTexture
    const float4* A;            // [H*W] plane RT_AOV_ALBEDO (coverage in .w)
    const float4* G;            // [H*W] plane RT_AOV_NORMAL_DEPTH
    const float4* Tp;           // [H*W] T' (rgb, a)
    const float*  Np;           // [H*W] N'
    const float4* Gp;           // [H*W] G' = (nc, zc) of the previous call
    float4* T;                  // [H*W] out
    float*  N;                  // [H*W] out
    float4* Gn;                 // [H*W] out: (nc, zc) of this call
    int W, H;
    float M[12];                // rows 0..2 of camLocalToWorld
    float O[3], V[3];           // worldSpaceCameraPos, viewParams
    float pc[3][3];             // c_i = column i of the upper 3 x 3 of M'
    float pcc[3];               // dot(c_i, c_i)
    float pt[3], pO[3], pV[3];  // t' = (M'[3], M'[7], M'[11]), O', V'
    float depthTol, normalTol2, maxHistory;     // depthTolerance, normalTolerance * normalTolerance, (float)maxHistory
};

__global__ __launch_bounds__(256) void k_temporal(TemporalArgs a)
{
    using namespace rtm;
    const int x = blockIdx.x * kTemporalTileW + (threadIdx.x & 63);
    const int y = blockIdx.y * kTemporalTileH + (threadIdx.x >> 6);         // (one row per wave)
    if (y >= a.H || x >= a.W) return;
    const size_t W = (size_t)a.W;
    const size_t pi = (size_t)y * W + (size_t)x;
    const float4 c = a.C[pi], g = a.G[pi];
    const float cov = a.A[pi].w;
    const bool surf = cov > 0.0f;
    const v3 nc = surf ? mk(g.x / cov, g.y / cov, g.z / cov) : mk(0.0f, 0.0f, 0.0f);
    const float zc = surf ? g.w / cov : 0.0f;
    // the centre ray (frag's, without jitter)
    const float Wf = (float)a.W, Hf = (float)a.H;
    const float uvx = ((float)x + 0.5f) / Wf, uvy = ((float)y + 0.5f) / Hf;
    const float lx = (uvx - 0.5f) * a.V[0], ly = (uvy - 0.5f) * a.V[1], lz = 1.0f * a.V[2];
    const float* M = a.M;
    const v3 F = mk(((M[0] * lx + M[1] * ly) + M[2]  * lz) + M[3]  * 1.0f,
                    ((M[4] * lx + M[5] * ly) + M[6]  * lz) + M[7]  * 1.0f,
                    ((M[8] * lx + M[9] * ly) + M[10] * lz) + M[11] * 1.0f);
    const v3 O = mk(a.O[0], a.O[1], a.O[2]);
    const v3 dir = normalize(F - O);
    // the point to reproject
    const v3 X = O + dir * zc;
    const v3 dO = X - mk(a.pO[0], a.pO[1], a.pO[2]);
    const float ze = __builtin_sqrtf(dot(dO, dO));
    const v3 q = surf ? X - mk(a.pt[0], a.pt[1], a.pt[2]) : dir;
    // into the previous camera
    const float l0 = dot(mk(a.pc[0][0], a.pc[0][1], a.pc[0][2]), q) / a.pcc[0];
    const float l1 = dot(mk(a.pc[1][0], a.pc[1][1], a.pc[1][2]), q) / a.pcc[1];
    const float l2 = dot(mk(a.pc[2][0], a.pc[2][1], a.pc[2][2]), q) / a.pcc[2];
    const float sc = a.pV[2] / l2;
    const float px = ((l0 * sc) / a.pV[0] + 0.5f) * Wf - 0.5f;
    const float py = ((l1 * sc) / a.pV[1] + 0.5f) * Hf - 0.5f;
    const bool valid = l2 > 0.0f && px > -1.0f && px < Wf && py > -1.0f && py < Hf;         // (NaN fails every comparison)
    const float x0f = __builtin_floorf(px), y0f = __builtin_floorf(py);
    const float fx = px - x0f, fy = py - y0f;
    const int x0 = valid ? (int)x0f : 0, y0 = valid ? (int)y0f : 0;        // valid: -1 <= x0 <= W - 1, -1 <= y0 <= H - 1
    // the twelve tap loads, together; a tap that cannot count loads this pixel's own address
    float4 tp[4], gp[4];
    float np[4];
    bool inside[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
        inside[k] = valid && tx >= 0 && tx < a.W && ty >= 0 && ty < a.H;
        const size_t ti = inside[k] ? (size_t)ty * W + (size_t)tx : pi;
        tp[k] = a.Tp[ti]; np[k] = a.Np[ti]; gp[k] = a.Gp[ti];
    }
    const float ztol = a.depthTol * ze;
    float sw = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f, hn = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float b = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        const float dnx = nc.x - gp[k].x, dny = nc.y - gp[k].y, dnz = nc.z - gp[k].z;
        const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
        const bool agrees = surf ? (gp[k].w > 0.0f && __builtin_fabsf(gp[k].w - ze) <= ztol && dn2 <= a.normalTol2) : gp[k].w == 0.0f;
        const bool counts = inside[k] && np[k] > 0.0f && agrees;
        sw = counts ? sw + b : sw;
        hx = counts ? hx + b * tp[k].x : hx; hy = counts ? hy + b * tp[k].y : hy; hz = counts ? hz + b * tp[k].z : hz;
        hn = counts ? hn + b * np[k] : hn;
    }
    // blend
    const float t = hn / sw + 1.0f;
    const float nb = t < a.maxHistory ? t : a.maxHistory;
    const float al = 1.0f / nb;
    const float om = 1.0f - al;
    const bool hist = sw >= 0.01f;
    float4 o;
    o.x = hist ? (hx / sw) * om + c.x * al : c.x;
    o.y = hist ? (hy / sw) * om + c.y * al : c.y;
    o.z = hist ? (hz / sw) * om + c.z * al : c.z;
    o.w = c.w;
    a.T[pi] = o;
    a.N[pi] = hist ? nb : 1.0f;
    a.Gn[pi] = make_float4(nc.x, nc.y, nc.z, zc);
}

} // namespace rtk
