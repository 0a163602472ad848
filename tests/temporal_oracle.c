/* temporal_oracle.c — the definition of temporal reprojection (include/rt.h "temporal reprojection") restated in plain C: the checker
 * the kernel is compared with bit for bit.  Test infrastructure only.  Compiled with the CFLAGS of oracle/Makefile (-ffp-contract=off,
 * no fast-math): every operation below is one IEEE float32 operation, in the order the header gives. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

typedef struct { float x, y, z; } v3;
static v3 V3(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static v3 sub(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static v3 normalize(v3 a)
{
    float len = sqrtf(dot(a, a));
    return V3(a.x / len, a.y / len, a.z / len);
}

/* One call.  C, A, G, Tp, Gp, T, Gn: H*W*4 floats, row 0 first; Np, N: H*W floats.  M / Mp: camLocalToWorld (16, row-major) of this
 * call and of the previous one, O / Op worldSpaceCameraPos, V / Vp viewParams.  have_history == 0 is call 0: N' reads as 0 everywhere
 * and the previous planes and camera are not looked at.  code (may be null): per pixel 3 ints, the decisions taken: bit 0 valid,
 * bits 1..4 tap k counts, bit 5 sw >= 0.01, bit 6 the history length was capped; then x0 and y0 (0 when not valid).
 * variant 0 = the definition; 1 = taps outside the image clamped to the border instead of skipped; 2 = no depth test; 3 = the history
 * length is not capped; 4 = t <= maxHistory for t < maxHistory in the cap (the same n at equality: only bit 6 of the code tells); 5 = the
 * depth test relative to G'.w instead of ze; 6 = no normal test: deliberate misreadings the tests must be able to tell apart. */
int temporal_step(const float* C, const float* A, const float* G, int W, int H,
                  const float* M, const float* O, const float* V, const float* Mp, const float* Op, const float* Vp,
                  const float* Tp, const float* Np, const float* Gp, int have_history,
                  int maxHistory, float depthTolerance, float normalTolerance, int variant,
                  float* T, float* N, float* Gn, int32_t* code)
{
    const float Wf = (float)W, Hf = (float)H;
    const float nt2 = normalTolerance * normalTolerance;
    const float mh = (float)maxHistory;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t pi = (size_t)y * W + x;
            const float* c = C + pi * 4;
            const float* g = G + pi * 4;
            const float cov = A[pi * 4 + 3];
            const int surf = cov > 0.0f;
            v3 nc = V3(0.0f, 0.0f, 0.0f);
            float zc = 0.0f;
            if (surf) { nc = V3(g[0] / cov, g[1] / cov, g[2] / cov); zc = g[3] / cov; }
            int32_t bits = 0, cx0 = 0, cy0 = 0;
            float sw = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f, hn = 0.0f;
            if (have_history) {
                const float uvx = ((float)x + 0.5f) / Wf, uvy = ((float)y + 0.5f) / Hf;
                const float lx = (uvx - 0.5f) * V[0], ly = (uvy - 0.5f) * V[1], lz = 1.0f * V[2];
                const v3 F = V3(((M[0] * lx + M[1] * ly) + M[2]  * lz) + M[3]  * 1.0f,
                                ((M[4] * lx + M[5] * ly) + M[6]  * lz) + M[7]  * 1.0f,
                                ((M[8] * lx + M[9] * ly) + M[10] * lz) + M[11] * 1.0f);
                const v3 o = V3(O[0], O[1], O[2]);
                const v3 dir = normalize(sub(F, o));
                v3 q = dir;
                float ze = 0.0f;
                if (surf) {
                    const v3 X = V3(o.x + dir.x * zc, o.y + dir.y * zc, o.z + dir.z * zc);
                    const v3 d = sub(X, V3(Op[0], Op[1], Op[2]));
                    q = sub(X, V3(Mp[3], Mp[7], Mp[11]));
                    ze = sqrtf(dot(d, d));
                }
                float l[3];
                for (int i = 0; i < 3; ++i) {
                    const v3 ci = V3(Mp[i], Mp[4 + i], Mp[8 + i]);
                    l[i] = dot(ci, q) / dot(ci, ci);
                }
                const float s = Vp[2] / l[2];
                const float px = ((l[0] * s) / Vp[0] + 0.5f) * Wf - 0.5f;
                const float py = ((l[1] * s) / Vp[1] + 0.5f) * Hf - 0.5f;
                const int valid = l[2] > 0.0f && px > -1.0f && px < Wf && py > -1.0f && py < Hf;
                if (valid) {
                    const float x0f = floorf(px), y0f = floorf(py);
                    const float fx = px - x0f, fy = py - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    bits |= 1; cx0 = x0; cy0 = y0;
                    const float ztol = depthTolerance * ze;
                    for (int j = 0; j < 2; ++j)
                        for (int i = 0; i < 2; ++i) {
                            int tx = x0 + i, ty = y0 + j;
                            const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                            if (tx < 0 || tx >= W || ty < 0 || ty >= H) {
                                if (variant != 1) continue;
                                tx = tx < 0 ? 0 : tx >= W ? W - 1 : tx;
                                ty = ty < 0 ? 0 : ty >= H ? H - 1 : ty;
                            }
                            const size_t ti = (size_t)ty * W + tx;
                            const float np = Np[ti];
                            const float* gp = Gp + ti * 4;
                            const float* tp = Tp + ti * 4;
                            if (!(np > 0.0f)) continue;
                            if (surf) {
                                const v3 e = sub(nc, V3(gp[0], gp[1], gp[2]));
                                if (!(gp[3] > 0.0f)) continue;
                                if (variant != 2 && !(fabsf(gp[3] - ze) <= (variant == 5 ? depthTolerance * gp[3] : ztol))) continue;
                                if (variant != 6 && !(dot(e, e) <= nt2)) continue;
                            } else if (!(gp[3] == 0.0f)) continue;
                            bits |= 2 << (j * 2 + i);
                            sw = sw + b;
                            hx = hx + b * tp[0]; hy = hy + b * tp[1]; hz = hz + b * tp[2];
                            hn = hn + b * np;
                        }
                }
            }
            float n = 1.0f;
            float* t = T + pi * 4;
            if (sw >= 0.01f) {
                const float tt = hn / sw + 1.0f;
                n = (variant == 4 ? tt <= mh : tt < mh) ? tt : mh;
                if (variant == 3) n = tt;
                bits |= 32;
                if (variant == 4 ? !(tt <= mh) : !(tt < mh)) bits |= 64;
                const float a = 1.0f / n;
                const float om = 1.0f - a;
                t[0] = (hx / sw) * om + c[0] * a;
                t[1] = (hy / sw) * om + c[1] * a;
                t[2] = (hz / sw) * om + c[2] * a;
            } else { t[0] = c[0]; t[1] = c[1]; t[2] = c[2]; }
            t[3] = c[3];
            N[pi] = n;
            Gn[pi * 4 + 0] = nc.x; Gn[pi * 4 + 1] = nc.y; Gn[pi * 4 + 2] = nc.z; Gn[pi * 4 + 3] = zc;
            if (code) { code[pi * 3] = bits; code[pi * 3 + 1] = cx0; code[pi * 3 + 2] = cy0; }
        }
    return 0;
}
