/* denoise_oracle.c — the denoiser's definition (include/rt.h "denoiser") restated in plain C: the checker the kernels are compared with
 * bit for bit.  Test infrastructure only.  Compiled with the CFLAGS of oracle/Makefile (-ffp-contract=off, no fast-math): every
 * operation below is one IEEE float32 operation, in the order the header gives. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* the exp2 polynomial of the library's math header, copied: floor(x + 0.5) split, degree-6 polynomial, two-step scaling */
static float floor_(float x)
{
    if (!(x > -2147483648.0f && x < 2147483648.0f)) return x;
    float t = (float)(int32_t)x;
    return t > x ? t - 1.0f : t;
}
static float exp2_(float x)
{
    if (x != x) return x;
    if (x >= 128.0f) return u2f(0x7f800000u);
    if (x < -150.0f) return 0.0f;
    float k = floor_(x + 0.5f);
    float f = x - k;
    float p = ((((1.535336188319500e-4f * f + 1.339887440266574e-3f) * f + 9.618437357674640e-3f) * f
                + 5.550332471162809e-2f) * f + 2.402264791363012e-1f) * f + 6.931472028550421e-1f;
    float r = p * f + 1.0f;
    int ki = (int)k;
    int k1 = ki >> 1, k2 = ki - k1;
    r = r * u2f((uint32_t)(k1 + 127) << 23);
    r = r * u2f((uint32_t)(k2 + 127) << 23);
    return r;
}
float denoise_exp2(float x) { return exp2_(x); }

/* C, A, G, out: H*W*4 floats, row 0 first.  variant 0 = the definition; 1 = taps outside the image clamped to the border instead of
 * skipped; 2 = a colour sigma that does not halve (kc_i = kc_0); 3 = d = max(A.ch + cov1, 0.01f) as a max that returns its NaN operand
 * (the definition's select gives 0.01f): deliberate misreadings the tests must be able to tell apart.
 * Returns 0, or -1 when memory runs out. */
int denoise_image(const float* C, const float* A, const float* G, int W, int H, int iterations, int demodulate,
                  float sigmaColour, float sigmaNormal, float sigmaDepth, int variant, float* out)
{
    static const float h[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
    const size_t n = (size_t)W * H;
    float* e = malloc((n ? n : 1) * 3 * sizeof(float));
    float* e2 = malloc((n ? n : 1) * 3 * sizeof(float));
    float* d = malloc((n ? n : 1) * 3 * sizeof(float));
    if (!e || !e2 || !d) { free(e); free(e2); free(d); return -1; }
    for (size_t i = 0; i < n; ++i) {
        const float cov1 = 1.0f - A[4 * i + 3];
        for (int ch = 0; ch < 3; ++ch) {
            float dv = 1.0f;
            if (demodulate) {
                const float t = A[4 * i + ch] + cov1;
                dv = variant == 3 ? (t < 0.01f ? 0.01f : t) : (t > 0.01f ? t : 0.01f);
                e[3 * i + ch] = C[4 * i + ch] / dv;
            } else e[3 * i + ch] = C[4 * i + ch];
            d[3 * i + ch] = dv;
        }
    }
    const float kn = 1.0f / (sigmaNormal * sigmaNormal);
    const float kz = 1.0f / (sigmaDepth * sigmaDepth);
    const float kc0 = 1.0f / (sigmaColour * sigmaColour);
    for (int it = 0; it < iterations; ++it) {
        const int s = 1 << it;
        const float kc = variant == 2 ? kc0 : kc0 * (float)(1 << (2 * it));
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                const float* gp = G + 4 * p;
                const float* ep = e + 3 * p;
                const float zs = kz / (gp[3] * gp[3] + 1e-6f);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        int qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
                            if (variant != 1) continue;
                            qx = qx < 0 ? 0 : qx >= W ? W - 1 : qx;
                            qy = qy < 0 ? 0 : qy >= H ? H - 1 : qy;
                        }
                        const size_t q = (size_t)qy * W + qx;
                        const float* gq = G + 4 * q;
                        const float* eq = e + 3 * q;
                        const float dnx = gp[0] - gq[0], dny = gp[1] - gq[1], dnz = gp[2] - gq[2];
                        const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
                        const float dz = gp[3] - gq[3];
                        const float dcx = ep[0] - eq[0], dcy = ep[1] - eq[1], dcz = ep[2] - eq[2];
                        const float dc2 = (dcx * dcx + dcy * dcy) + dcz * dcz;
                        const float xx = (dn2 * kn + (dz * dz) * zs) + dc2 * kc;
                        const float w = (h[dy + 2] * h[dx + 2]) * exp2_(-xx);
                        sw = sw + w;
                        sx = sx + w * eq[0]; sy = sy + w * eq[1]; sz = sz + w * eq[2];
                    }
                e2[3 * p + 0] = sx / sw; e2[3 * p + 1] = sy / sw; e2[3 * p + 2] = sz / sw;
            }
        float* t = e; e = e2; e2 = t;
    }
    for (size_t i = 0; i < n; ++i) {
        for (int ch = 0; ch < 3; ++ch) out[4 * i + ch] = e[3 * i + ch] * d[3 * i + ch];
        out[4 * i + 3] = C[4 * i + 3];
    }
    free(e); free(e2); free(d);
    return 0;
}
