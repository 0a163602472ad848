/* vdenoise_oracle.c — the variance-guided denoiser's definition (include/rt.h "variance-guided denoiser") restated in plain C: the
 * checker the kernels are compared with bit for bit.  Test infrastructure only.  Compiled with the CFLAGS of oracle/Makefile
 * (-ffp-contract=off, no fast-math): every operation below is one IEEE float32 operation, in the order the header gives. */
#include <math.h>
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
float vdenoise_exp2(float x) { return exp2_(x); }

static float lum(const float* e) { return (0.2126f * e[0] + 0.7152f * e[1]) + 0.0722f * e[2]; }

/* Planes of H*W pixels, row 0 first: e = 3 floats per pixel, G = 4, var = 1.
 * variant 0 = the definition; deliberate misreadings the tests must be able to tell apart: 1 = taps outside the image clamped to the
 * border instead of skipped (estimate, prefilter and passes), 2 = the prefilter at spacing s instead of 1, 3 = the variance weighted by
 * w instead of w*w (var_{i+1} = sv / sw), 4 = d = max(A.ch + cov1, 0.01f) as a max that returns its NaN operand (the definition's select
 * gives 0.01f), 5 = var_0 = max(v, 0) as a max that returns its NaN operand (the definition's select gives 0). */

/* var_0 from e0 */
static void estimate(const float* e, const float* G, int W, int H, float kn, float kz, int variant, float* var)
{
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            const float* gp = G + 4 * p;
            const float zs = kz / (gp[3] * gp[3] + 1e-6f);
            float sg = 0.0f, m1 = 0.0f, m2 = 0.0f;
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
                        if (variant != 1) continue;
                        qx = qx < 0 ? 0 : qx >= W ? W - 1 : qx;
                        qy = qy < 0 ? 0 : qy >= H ? H - 1 : qy;
                    }
                    const size_t q = (size_t)qy * W + qx;
                    const float* gq = G + 4 * q;
                    const float dnx = gp[0] - gq[0], dny = gp[1] - gq[1], dnz = gp[2] - gq[2];
                    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
                    const float dz = gp[3] - gq[3];
                    const float g = exp2_(-(dn2 * kn + (dz * dz) * zs));
                    const float lq = lum(e + 3 * q);
                    sg = sg + g;
                    m1 = m1 + g * lq;
                    m2 = m2 + g * (lq * lq);
                }
            const float mu = m1 / sg;
            const float v = m2 / sg - mu * mu;
            var[p] = variant == 5 ? (v < 0.0f ? 0.0f : v) : (v > 0.0f ? v : 0.0f);
        }
}

/* one pass at spacing s: (e, var) -> (e2, var2) */
static void pass(const float* e, const float* var, const float* G, int W, int H, int s, float sl, float kn, float kz, int variant,
                 float* e2, float* var2)
{
    static const float h[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
    static const float k3[3] = { 1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f };
    const int ps = variant == 2 ? s : 1;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            const float* gp = G + 4 * p;
            const float* ep = e + 3 * p;
            const float zs = kz / (gp[3] * gp[3] + 1e-6f);
            float pn = 0.0f, pd = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    int qx = x + dx * ps, qy = y + dy * ps;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
                        if (variant != 1) continue;
                        qx = qx < 0 ? 0 : qx >= W ? W - 1 : qx;
                        qy = qy < 0 ? 0 : qy >= H ? H - 1 : qy;
                    }
                    pn = pn + (k3[dy + 1] * k3[dx + 1]) * var[(size_t)qy * W + qx];
                    pd = pd + k3[dy + 1] * k3[dx + 1];
                }
            const float gv = pn / pd;
            const float kl = 1.0f / (sl * sqrtf(gv) + 1e-6f);
            const float lp = lum(ep);
            float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
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
                    const float xx = (dn2 * kn + (dz * dz) * zs) + fabsf(lp - lum(eq)) * kl;
                    const float w = (h[dy + 2] * h[dx + 2]) * exp2_(-xx);
                    sw = sw + w;
                    sx = sx + w * eq[0]; sy = sy + w * eq[1]; sz = sz + w * eq[2];
                    sv = sv + (variant == 3 ? w : w * w) * var[q];
                }
            e2[3 * p + 0] = sx / sw; e2[3 * p + 1] = sy / sw; e2[3 * p + 2] = sz / sw;
            var2[p] = variant == 3 ? sv / sw : sv / (sw * sw);
        }
}

/* prep: e0 (3 floats per pixel) and d (3 floats per pixel) from C and A (4 floats per pixel) */
static void prep(const float* C, const float* A, size_t n, int demodulate, int variant, float* e, float* d)
{
    for (size_t i = 0; i < n; ++i) {
        const float cov1 = 1.0f - A[4 * i + 3];
        for (int ch = 0; ch < 3; ++ch) {
            float dv = 1.0f;
            if (demodulate) {
                const float t = A[4 * i + ch] + cov1;
                dv = variant == 4 ? (t < 0.01f ? 0.01f : t) : (t > 0.01f ? t : 0.01f);
                e[3 * i + ch] = C[4 * i + ch] / dv;
            } else e[3 * i + ch] = C[4 * i + ch];
            d[3 * i + ch] = dv;
        }
    }
}

/* The whole image: C, A, G, out H*W*4 floats, var0 (may be NULL) H*W floats.  Returns 0, or -1 when memory runs out. */
int vdenoise_image(const float* C, const float* A, const float* G, int W, int H, int iterations, int demodulate,
                   float sigmaLuminance, float sigmaNormal, float sigmaDepth, int variant, float* out, float* var0)
{
    const size_t n = (size_t)W * H, m = n ? n : 1;
    float* e = malloc(m * 3 * sizeof(float));
    float* e2 = malloc(m * 3 * sizeof(float));
    float* d = malloc(m * 3 * sizeof(float));
    float* v = malloc(m * sizeof(float));
    float* v2 = malloc(m * sizeof(float));
    if (!e || !e2 || !d || !v || !v2) { free(e); free(e2); free(d); free(v); free(v2); return -1; }
    prep(C, A, n, demodulate, variant, e, d);
    const float kn = 1.0f / (sigmaNormal * sigmaNormal);
    const float kz = 1.0f / (sigmaDepth * sigmaDepth);
    estimate(e, G, W, H, kn, kz, variant, v);
    if (var0) memcpy(var0, v, n * sizeof(float));
    for (int it = 0; it < iterations; ++it) {
        pass(e, v, G, W, H, 1 << it, sigmaLuminance, kn, kz, variant, e2, v2);
        float* t = e; e = e2; e2 = t;
        t = v; v = v2; v2 = t;
    }
    for (size_t i = 0; i < n; ++i) {
        for (int ch = 0; ch < 3; ++ch) out[4 * i + ch] = e[3 * i + ch] * d[3 * i + ch];
        out[4 * i + 3] = C[4 * i + 3];
    }
    free(e); free(e2); free(d); free(v); free(v2);
    return 0;
}

/* var_0 alone */
int vdenoise_variance(const float* C, const float* A, const float* G, int W, int H, int demodulate, float sigmaNormal, float sigmaDepth,
                      int variant, float* var0)
{
    const size_t n = (size_t)W * H, m = n ? n : 1;
    float* e = malloc(m * 3 * sizeof(float));
    float* d = malloc(m * 3 * sizeof(float));
    if (!e || !d) { free(e); free(d); return -1; }
    prep(C, A, n, demodulate, variant, e, d);
    estimate(e, G, W, H, 1.0f / (sigmaNormal * sigmaNormal), 1.0f / (sigmaDepth * sigmaDepth), variant, var0);
    free(e); free(d);
    return 0;
}

/* one pass from injected (e_i, var_i): e and e_out H*W*3 floats, var and var_out H*W floats */
int vdenoise_pass(const float* e, const float* var, const float* G, int W, int H, int step, float sigmaLuminance, float sigmaNormal,
                  float sigmaDepth, int variant, float* e_out, float* var_out)
{
    pass(e, var, G, W, H, step, sigmaLuminance, 1.0f / (sigmaNormal * sigmaNormal), 1.0f / (sigmaDepth * sigmaDepth), variant, e_out, var_out);
    return 0;
}
